"""Golden values for the evaluation metrics, generated FROM THE REFERENCE.

Runs only in the build container: imports the reference's metrics package on the CPU (metric_utils,
precision_recall, frechet_inception_distance; not metric_main, which needs open_clip), replaces its two feature
sweeps by functions that return its own FeatureStats filled from the fixtures of tests/metrics_cases.py, and
records what its code computes with num_gpus = 1:
  * lattice cases: compute_pr's precision / recall, and, from its compute_distances, the fp16 radii and the
    `pred` vectors of both directions (their means are checked against compute_pr's return);
  * FeatureStats: raw_mean / raw_cov / mean / cov after 7 uneven appends of the integer and the float fixture;
  * compute_fid on the stand-in detector's features, appended in 7 chunks and in 1 chunk.
Fixture conditions asserted here: lattice precision and recall in [0.2, 0.8] with at least 50 pairs d == r;
at most 1 % of the Gaussian radii rows excused by the fp64 criterion alone.
Writes tests/golden/metrics_golden.npz.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("VFM_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)

import metrics_cases as mc  # noqa: E402
from metrics import metric_utils as ref_mu  # noqa: E402
from metrics import precision_recall as ref_pr  # noqa: E402
from metrics import frechet_inception_distance as ref_fid  # noqa: E402

assert os.path.abspath(ref_mu.__file__).startswith(os.path.abspath(REF))
OUT = mc.GOLDEN
CPU = torch.device("cpu")
arrays, meta = {}, {"lattice": [], "gauss": {}}


def ref_stats(x, sizes=None, **kw):
    s = ref_mu.FeatureStats(**kw)
    for part in (mc.chunks(x, sizes) if sizes else [x]):
        s.append(part)
    return s


def patch_sweeps(real, gen, sizes):
    """The reference's sweeps return its FeatureStats over the fixture features."""
    def for_dataset(opts, detector_url, detector_kwargs={}, max_items=None, shuffle_size=None, rel_lo=0, rel_hi=1,
                    **stats_kwargs):
        return ref_stats(real, sizes, **stats_kwargs)

    def for_generator(opts, detector_url, detector_kwargs, rel_lo=0, rel_hi=1, **stats_kwargs):
        return ref_stats(gen, sizes, **stats_kwargs)
    ref_mu.compute_feature_stats_for_dataset = for_dataset
    ref_mu.compute_feature_stats_for_generator = for_generator


opts = ref_mu.MetricOptions(num_gpus=1, rank=0, device=CPU, cache=False)

# ---- lattice precision / recall
for case in mc.LATTICE:
    N, M, D, C, seed = case
    real, gen = mc.lattice(*case)
    patch_sweeps(real, gen, None)
    precision, recall = ref_pr.compute_pr(opts, max_real=N, num_gen=M, nhood_size=mc.NHOOD, row_batch_size=10000,
                                          col_batch_size=10000)
    t = mc.tag(case)
    r16, g16 = torch.from_numpy(real).to(torch.float16), torch.from_numpy(gen).to(torch.float16)
    ties = 0
    for name, manifold, probes, want in (("precision", r16, g16, precision), ("recall", g16, r16, recall)):
        dist = ref_pr.compute_distances(manifold, manifold, 1, 0, 10000)
        kth = dist.to(torch.float32).kthvalue(mc.NHOOD + 1).values.to(torch.float16)
        dist = ref_pr.compute_distances(probes, manifold, 1, 0, 10000)
        pred = (dist <= kth).any(dim=1)
        assert float(pred.to(torch.float32).mean()) == want
        ties += int((dist == kth.float()).sum())
        arrays[f"{t}/{name}/radii"] = kth.numpy()
        arrays[f"{t}/{name}/pred"] = pred.numpy()
        arrays[f"{t}/{name}"] = np.float64(want)
    assert 0.2 <= precision <= 0.8 and 0.2 <= recall <= 0.8 and ties >= 50, (case, precision, recall, ties)
    meta["lattice"].append(dict(case=case, precision=precision, recall=recall, ties=ties))
    print(t, f"precision {precision:.3f} recall {recall:.3f} pairs d == r {ties}")

# ---- Gaussian fixtures: the share the fp64 criterion alone excuses
feats, _ = mc.gaussian(mc.GAUSS_RADII[0], 1, mc.GAUSS_RADII[1], mc.GAUSS_RADII[2])
_, excused = mc.radius_rule(feats, mc.NHOOD)
share = float(excused.double().mean())
assert share <= 0.01, share
meta["gauss"]["radii_excused_share"] = share
manifold, probes = mc.gaussian(*mc.GAUSS_HITS)
radii, _ = mc.radius_rule(manifold, mc.NHOOD)
expect, excused = mc.hits_rule(probes, manifold, radii)
meta["gauss"]["hits_excused_share"] = float(excused.double().mean())
meta["gauss"]["precision64"] = float(expect.double().mean())
assert meta["gauss"]["hits_excused_share"] <= 0.01
print("gaussian", meta["gauss"])

# ---- FeatureStats
for kind in ("int", "float"):
    x = mc.stats_fixture(kind)
    s = ref_stats(x, mc.CHUNKS, capture_mean_cov=True)
    mean, cov = s.get_mean_cov()
    arrays[f"stats/{kind}/raw_mean"], arrays[f"stats/{kind}/raw_cov"] = s.raw_mean, s.raw_cov
    arrays[f"stats/{kind}/mean"], arrays[f"stats/{kind}/cov"] = mean, cov

# ---- compute_fid on the stand-ins' features
real, gen = mc.fid_features()
n = real.shape[0]
sizes7 = [1, 9, 32, 3, 25, 16, n - 86]
for name, sizes in (("fid7", sizes7), ("fid1", None)):
    patch_sweeps(real, gen, sizes)
    arrays[f"fid/{name}"] = np.float64(ref_fid.compute_fid(opts, max_real=None, num_gen=n))
for name, x in (("real", real), ("gen", gen)):
    mean, cov = ref_stats(x, sizes7, capture_mean_cov=True).get_mean_cov()
    arrays[f"fid/mu_{name}"], arrays[f"fid/sigma_{name}"] = mean, cov
meta["fid"] = dict(fid7=float(arrays["fid/fid7"]), fid1=float(arrays["fid/fid1"]),
                   moved=abs(float(arrays["fid/fid7"]) - float(arrays["fid/fid1"])))
print("fid", meta["fid"])

arrays["meta"] = np.array(json.dumps(meta))
np.savez_compressed(OUT, **arrays)
print(f"wrote {OUT}: {len(arrays)} arrays, {os.path.getsize(OUT) / 1024:.1f} KiB")
