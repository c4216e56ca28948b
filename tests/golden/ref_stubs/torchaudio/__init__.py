"""Stand-in for torchaudio (not installed): the reference's tools/evaluate_alignment/metrics.py imports
`torchaudio.functional` at module level and touches it only in the commented-out edit_distance_knn metric."""
from . import functional  # noqa: F401
