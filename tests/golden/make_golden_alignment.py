"""Golden values for the alignment metrics, generated FROM THE REFERENCE.

Runs only in the build container: imports /root/reference's tools/evaluate_alignment/metrics.py on the CPU
(torchaudio, which it imports and never uses on these paths, comes from ref_stubs) and records, for the four
gap-safe cases (n, d, k, seed) of tests/alignment_cases.py:
  * the two normalised fp32 feature matrices,
  * the reference's cknna / mutual_knn / cycle_knn on the features in fp64, and its cknna in fp32,
and, for one raw feature pair with outliers saved as the extractors' .pt payload, the output of the
reference's load_and_process_features (its `.cuda()` made a no-op: there is no GPU here).
Writes tests/golden/alignment_golden.npz.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_alignment.py
"""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("VFM_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, "ref_stubs"))
sys.path.insert(0, os.path.dirname(HERE))

import alignment_cases as ac  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_alignment_metrics",
                                              os.path.join(REF, "tools", "evaluate_alignment", "metrics.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

OUT = os.path.join(HERE, "alignment_golden.npz")
arrays, meta = {}, {"cases": []}

for n, d, k, seed in ac.GAP_SAFE:
    a, b = ac.make_features(n, d, seed)
    gap = min(ac.min_boundary_gap(a, k), ac.min_boundary_gap(b, k))
    assert gap >= 10 * ac.tol(d), (n, d, k, seed, gap)
    tag = ac.tag(n, d, k, seed)
    arrays[f"{tag}/A"] = a.numpy()
    arrays[f"{tag}/B"] = b.numpy()
    a64, b64 = a.double(), b.double()
    arrays[f"{tag}/cknna64"] = np.float64(ref.AlignmentMetrics.cknna(a64, b64, topk=k))
    arrays[f"{tag}/cknna32"] = np.float64(ref.AlignmentMetrics.cknna(a, b, topk=k))
    arrays[f"{tag}/mutual_knn"] = np.float64(ref.AlignmentMetrics.mutual_knn(a64, b64, topk=k))
    arrays[f"{tag}/cycle_knn"] = np.float64(ref.AlignmentMetrics.cycle_knn(a64, b64, topk=k))
    meta["cases"].append({"n": n, "d": d, "k": k, "seed": seed, "min_gap": gap})
    print(tag, {key.split("/")[1]: float(v) for key, v in arrays.items() if key.startswith(tag) and v.ndim == 0},
          f"gap {gap:.3e} = {gap / ac.tol(d):.1f} tol")

# ---- the preparation pipeline on a raw pair with outliers
raw1, raw2 = ac.make_raw_pair()
torch.Tensor.cuda = lambda self, *a, **kw: self
with tempfile.TemporaryDirectory() as tmp:
    paths = []
    for i, raw in enumerate((raw1, raw2)):
        p = os.path.join(tmp, f"f{i}.pt")
        names = [f"img{j:04d}" for j in range(raw.shape[0])]
        torch.save({"features": raw, "names": names, "transformations": [{"mode": "clean"}] * len(names)}, p)
        paths.append(p)
    fa, fb = ref.load_and_process_features(*paths)
arrays["prep/raw1"], arrays["prep/raw2"] = raw1.numpy(), raw2.numpy()
arrays["prep/out1"], arrays["prep/out2"] = fa.numpy(), fb.numpy()

arrays["meta"] = np.array(json.dumps(meta))
np.savez_compressed(OUT, **arrays)
print(f"wrote {OUT}: {len(arrays)} arrays, {os.path.getsize(OUT) / 1024:.1f} KiB")
