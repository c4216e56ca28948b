"""Evaluation metrics (reference `metrics/`): reconstruction FID and improved precision / recall over a
feature detector found on the local disk, their statistics on the fidstats / prknn kernels."""
