"""The metric kernels on the GPU: csrc/fidstats.hip behind torch_utils/ops/fidstats_hip.py and csrc/prknn.hip behind
torch_utils/ops/prknn_hip.py, and the metrics package on top of them.

References: numpy fp64 for the statistics (bit-equal on integer input; within 2 n 2^-53 (|X|^T |X|)_ij on randn,
metrics_cases.cov_bound); the reference's own radii / pred vectors / precision / recall on the lattice cases
(tests/golden/metrics_golden.npz: every path must agree bit for bit there); the fp64 restatement with the fp32
error band on the Gaussian cases (metrics_cases.radius_rule / hits_rule, at most 1 % of rows excused)."""
import functools
import warnings

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import metrics_cases as mc
from test_no_host_sync_gpu import _sync_watch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 64                                             # guard doubles after each statistics buffer


@functools.lru_cache(maxsize=None)
def _gold():
    return mc.golden()


def _fid():
    from torch_utils.ops import fidstats_hip
    return fidstats_hip


def _pr():
    from torch_utils.ops import prknn_hip
    return prknn_hip


class _Record(TorchDispatchMode):
    """The aten calls that would run a vendor GEMM, a cdist kernel or a device selection."""
    BAD = ("aten.mm", "aten.matmul", "aten.bmm", "aten.addmm", "aten.cdist", "aten._cdist", "aten._euclidean_dist",
           "aten.kthvalue", "aten.topk", "aten.sort")

    def __init__(self):
        super().__init__()
        self.hits = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if str(func).startswith(self.BAD):
            self.hits.append(str(func))
        return func(*args, **(kwargs or {}))


# ---------------------------------------------------------------------------------------------- accumulate

def _batches(n, D, kind, dtype):
    """Three batches [n, D] (the second a strided view) on the CPU, values exact in `dtype`."""
    rng = np.random.default_rng(n * 10007 + D)
    out = []
    for i in range(3):
        if kind == "int":
            x = rng.integers(-8, 9, (n, D)).astype(np.float32)
        else:
            x = rng.standard_normal((n, D)).astype(np.float32)
        out.append(torch.from_numpy(x).to(dtype))
    return out


def _run_accumulate(batches, D):
    """(raw_mean, raw_cov) after the three appends, with the guards checked."""
    buf_m = torch.full([D + GUARD], -7.0, dtype=torch.float64, device=DEV)
    buf_c = torch.full([D * D + GUARD], -7.0, dtype=torch.float64, device=DEV)
    mean, cov = buf_m[:D].zero_(), buf_c[:D * D].view(D, D).zero_()
    for i, x in enumerate(batches):
        xd = x.to(DEV)
        if i == 1:                                     # a strided input: columns 3 .. 3 + D of a wider matrix
            wide = torch.zeros(x.shape[0], D + 9, dtype=x.dtype, device=DEV)
            wide[:, 3:3 + D] = xd
            xd = wide[:, 3:3 + D]
            assert xd.stride(0) == D + 9
        _fid().accumulate(mean, cov, xd)
    assert bool((buf_m[D:] == -7.0).all()) and bool((buf_c[D * D:] == -7.0).all())
    return mean.cpu().numpy(), cov.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("n,D", [(1, 5), (64, 2048), (67, 200), (1024, 130)])
def test_accumulate_integer_input_bit_equal(n, D, dtype):
    batches = _batches(n, D, "int", dtype)
    with _Record() as rec:
        mean, cov = _run_accumulate(batches, D)
    assert rec.hits == [], rec.hits
    x64 = [b.double().numpy() for b in batches]
    assert np.array_equal(mean, sum(x.sum(axis=0) for x in x64))
    assert np.array_equal(cov, sum(x.T @ x for x in x64))
    mean2, cov2 = _run_accumulate(batches, D)          # two runs are bitwise identical
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("n,D", [(1, 5), (64, 2048), (67, 200), (1024, 130)])
def test_accumulate_randn_within_the_rounding_bound(n, D, dtype):
    batches = _batches(n, D, "float", dtype)
    mean, cov = _run_accumulate(batches, D)
    xs = np.concatenate([b.double().numpy() for b in batches])
    err = np.abs(cov - xs.T @ xs)
    bound = mc.cov_bound(xs) + 2.0 ** -1000
    print(f"max err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert (np.abs(mean - xs.sum(axis=0)) <= 2 * xs.shape[0] * 2.0 ** -53 * np.abs(xs).sum(axis=0)).all()
    mean2, cov2 = _run_accumulate(batches, D)
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2)
    _fid().set_force_ref(True)                         # the torch path on the GPU obeys the same bound
    try:
        with _Record() as rec:
            _, cov3 = _run_accumulate(batches, D)
        assert any(h.startswith("aten.mm") for h in rec.hits)
    finally:
        _fid().set_force_ref(False)
    assert (np.abs(cov3 - xs.T @ xs) <= bound).all()


# ---------------------------------------------------------------------------------------------- knn_radius

@functools.lru_cache(maxsize=None)
def _lattice16(case):
    real, gen = mc.lattice(*case)
    return torch.from_numpy(real).to(torch.float16), torch.from_numpy(gen).to(torch.float16)


@pytest.mark.parametrize("case", mc.LATTICE, ids=mc.tag)
def test_knn_radius_lattice_bit_equal_and_split_independent(case):
    g, t = _gold(), mc.tag(case)
    for name, feats in zip(("precision", "recall"), _lattice16(case)):
        want = torch.from_numpy(g[f"{t}/{name}/radii"])
        fd = feats.to(DEV)
        with _Record() as rec:
            got = _pr().knn_radius(fd, mc.NHOOD)
        assert rec.hits == [], rec.hits
        assert got.dtype == torch.float16 and got.is_cuda and torch.equal(got.cpu(), want)
        for splits in (1, 2, 5):
            assert torch.equal(_pr().knn_radius(fd, mc.NHOOD, splits=splits).cpu(), want)
        assert torch.equal(_pr().knn_radius(fd, mc.NHOOD, rows=(130, 251)).cpu(), want[130:251])
        _pr().set_force_ref(True)                      # the torch path on the GPU: the same bits
        try:
            assert torch.equal(_pr().knn_radius(fd, mc.NHOOD).cpu(), want)
        finally:
            _pr().set_force_ref(False)


def test_knn_radius_gaussian_follows_the_rounding_rule():
    feats, _ = mc.gaussian(mc.GAUSS_RADII[0], 1, mc.GAUSS_RADII[1], mc.GAUSS_RADII[2])
    got = _pr().knn_radius(feats.to(DEV), mc.NHOOD)
    share = mc.check_radii(got, feats, mc.NHOOD, cap=0.01)
    print(f"excused rows {share:.4%}")
    for splits in (1, 3):
        assert torch.equal(_pr().knn_radius(feats.to(DEV), mc.NHOOD, splits=splits), got)


def test_knn_radius_vgg_width():
    """N = 257, D = 4096 against the fp64 restatement: exact outside the band, one fp16 step inside it. At this
    width the band is wider than the fp16 spacing for most rows, so the 1 % cap of the D = 32 fixture does not
    apply here; every row is still held to one step."""
    N, D, seed = mc.WIDE
    g = torch.Generator().manual_seed(seed)
    feats = (0.5 * torch.randn(N, D, generator=g)).to(torch.float16)
    got = _pr().knn_radius(feats.to(DEV), mc.NHOOD)
    share = mc.check_radii(got, feats, mc.NHOOD, cap=None)
    print(f"excused rows {share:.4%}")
    assert torch.equal(_pr().knn_radius(feats.to(DEV), mc.NHOOD, splits=3), got)


@pytest.mark.parametrize("N,D,k", [(4, 8, 3), (2, 5, 1), (1, 3, 0), (64, 13, 63), (129, 40, 3)])
def test_knn_radius_smallest_n_and_odd_widths(N, D, k):
    """N = k + 1 (the radius is the largest distance of the row), D with no 16-byte rows (the element path), a
    K-tile with a tail, k + 1 = 64 (the list bound): integer features, so the torch path on the CPU is exact."""
    g = torch.Generator().manual_seed(N * 100 + D)
    feats = torch.randint(-5, 6, (N, D), generator=g).to(torch.float16)
    want = _pr().knn_radius(feats, k)
    got = _pr().knn_radius(feats.to(DEV), k)
    assert torch.equal(got.cpu(), want)
    if N == k + 1:
        d2 = (feats.float()[:, None, :] - feats.float()[None, :, :]).pow(2).sum(-1)      # exact integers
        assert torch.equal(got.cpu(), d2.sqrt().max(dim=1).values.to(torch.float16))
    with pytest.raises(ValueError):
        _pr().knn_radius(feats.to(DEV), N)             # k + 1 > N
    wide = torch.zeros(N, D + 11, dtype=torch.float16, device=DEV)
    wide[:, 2:2 + D] = feats.to(DEV)
    assert torch.equal(_pr().knn_radius(wide[:, 2:2 + D], k).cpu(), want)     # a leading dimension


def test_knn_radius_past_the_list_bound_takes_the_torch_path():
    g = torch.Generator().manual_seed(0)
    feats = torch.randint(-5, 6, (100, 16), generator=g).to(torch.float16)
    with _Record() as rec:
        got = _pr().knn_radius(feats.to(DEV), 64)      # k + 1 = 65
    assert any(h.startswith("aten.kthvalue") for h in rec.hits)
    assert torch.equal(got.cpu(), _pr().knn_radius(feats, 64))


# ------------------------------------------------------------------------------------------- manifold_hits

@pytest.mark.parametrize("case", mc.LATTICE, ids=mc.tag)
def test_manifold_hits_lattice_bit_equal_both_directions(case):
    g, t = _gold(), mc.tag(case)
    real, gen = _lattice16(case)
    for name, manifold, probes in (("precision", real, gen), ("recall", gen, real)):
        radii = torch.from_numpy(g[f"{t}/{name}/radii"]).to(DEV)
        want = torch.from_numpy(g[f"{t}/{name}/pred"])
        with _Record() as rec:
            hits, mean = _pr().manifold_hits(probes.to(DEV), manifold.to(DEV), radii)
        assert rec.hits == [], rec.hits
        assert hits.dtype == torch.bool and mean.is_cuda and mean.dtype == torch.float32
        assert torch.equal(hits.cpu(), want) and float(mean) == float(g[f"{t}/{name}"])
        for splits in (1, 2, 5):
            h2, m2 = _pr().manifold_hits(probes.to(DEV), manifold.to(DEV), radii, splits=splits)
            assert torch.equal(h2.cpu(), want) and float(m2) == float(mean)
        h1, m1 = _pr().manifold_hits(probes[7:8].to(DEV), manifold.to(DEV), radii)      # P = 1
        assert h1.tolist() == [bool(want[7])] and float(m1) == float(want[7])


def test_manifold_hits_early_exit_is_not_observable():
    """Every row hits in the first column tile; no row hits at all; only the very last column can hit."""
    real, gen = _lattice16(mc.LATTICE[1])
    manifold, N = real.to(DEV), real.shape[0]
    big = torch.full([N], 1000.0, dtype=torch.float16, device=DEV)
    zero = torch.zeros([N], dtype=torch.float16, device=DEV)
    far = (gen + 40).to(DEV)                           # no row of `far` equals a manifold row
    for splits in (0, 1, 3):
        hits, mean = _pr().manifold_hits(gen.to(DEV), manifold, big, splits=splits)
        assert bool(hits.all()) and float(mean) == 1.0
        hits, mean = _pr().manifold_hits(far, manifold, zero, splits=splits)
        assert not bool(hits.any()) and float(mean) == 0.0
        last = zero.clone()
        last[N - 1] = 1000.0
        hits, mean = _pr().manifold_hits(far, manifold, last, splits=splits)
        assert bool(hits.all()) and float(mean) == 1.0
        probes = torch.cat([real[:5], (gen + 40)[:6]]).to(DEV)      # rows 0-4 are manifold rows: d = 0 <= 0
        hits, mean = _pr().manifold_hits(probes, manifold, zero, splits=splits)
        assert hits.tolist() == [True] * 5 + [False] * 6 and float(mean) == float(np.float32(5) / np.float32(11))


def test_manifold_hits_gaussian_follows_the_rounding_rule():
    manifold, probes = mc.gaussian(*mc.GAUSS_HITS)
    radii, _ = mc.radius_rule(manifold, mc.NHOOD)      # fp64-derived radii, passed in
    expect, excused = mc.hits_rule(probes, manifold, radii)
    hits, mean = _pr().manifold_hits(probes.to(DEV), manifold.to(DEV), radii.to(DEV))
    share = float(excused.double().mean())
    print(f"precision {float(mean):.4f} fp64 {float(expect.double().mean()):.4f} excused rows {share:.4%}")
    assert share <= 0.01
    assert torch.equal(hits.cpu()[~excused], expect[~excused])
    assert float(mean) == float(hits.cpu().to(torch.float32).mean())
    h3, m3 = _pr().manifold_hits(probes.to(DEV), manifold.to(DEV), radii.to(DEV), splits=4)
    assert torch.equal(h3, hits) and float(m3) == float(mean)


# --------------------------------------------------------------------------------------------- path checks

@pytest.mark.parametrize("case", mc.LATTICE, ids=mc.tag)
def test_compute_pr_on_the_gpu_equals_the_reference(case, monkeypatch):
    from metrics import metric_utils, precision_recall
    real, gen = mc.lattice(*case)
    g, t = _gold(), mc.tag(case)

    def stats(x):
        s = metric_utils.FeatureStats(capture_all=True)
        for part in (x[:100], x[100:]):
            s.append_torch(torch.from_numpy(part).to(DEV))
        return s
    monkeypatch.setattr(metric_utils, "compute_feature_stats_for_dataset", lambda **kw: stats(real))
    monkeypatch.setattr(metric_utils, "compute_feature_stats_for_generator", lambda **kw: stats(gen))
    opts = metric_utils.MetricOptions(num_gpus=1, rank=0, device=DEV)
    with _Record() as rec:
        precision, recall = precision_recall.compute_pr(opts, max_real=case[0], num_gen=case[1], nhood_size=mc.NHOOD,
                                                        row_batch_size=10000, col_batch_size=10000)
    assert rec.hits == [], rec.hits
    assert precision == float(g[f"{t}/precision"]) and recall == float(g[f"{t}/recall"])


def test_append_torch_keeps_the_statistics_on_the_device_without_host_syncs():
    from metrics import metric_utils
    x = mc.stats_fixture("int")
    parts = [torch.from_numpy(p).to(DEV) for p in mc.chunks(x)]
    s = metric_utils.FeatureStats(capture_all=True, capture_mean_cov=True, max_items=190)
    s.append_torch(parts[0])                           # first call: buffers created, library loaded
    torch.cuda.synchronize()
    with _sync_watch() as hits, _Record() as rec:
        for p in parts[1:]:
            s.append_torch(p)
    assert hits == [], hits
    assert rec.hits == [], rec.hits
    assert s.raw_mean.is_cuda and s.raw_cov.is_cuda and s.get_all_torch().is_cuda and s.num_items == 190
    ref = metric_utils.FeatureStats(capture_all=True, capture_mean_cov=True, max_items=190)
    for p in mc.chunks(x):
        ref.append(p)
    mean, cov = s.get_mean_cov()
    rmean, rcov = ref.get_mean_cov()
    assert np.array_equal(mean, rmean) and np.array_equal(cov, rcov) and np.array_equal(s.get_all(), ref.get_all())


def test_kernel_timer_regions():
    """The three regions are registered and timed under their rocprof kernel names."""
    from torch_utils.ops import kernel_timer
    assert kernel_timer.rocprof_name("feature_stats_accum<f32>") == "xtx_kernel<float>"
    assert kernel_timer.rocprof_name("knn_radius<f16>") == "dist_kernel<0>"
    assert kernel_timer.rocprof_name("manifold_hits<f16>") == "dist_kernel<1>"
    real, gen = _lattice16(mc.LATTICE[0])
    kernel_timer.enable(True)
    try:
        radii = _pr().knn_radius(real.to(DEV), mc.NHOOD)
        _pr().manifold_hits(gen.to(DEV), real.to(DEV), radii)
        mean = torch.zeros(8, dtype=torch.float64, device=DEV)
        cov = torch.zeros(8, 8, dtype=torch.float64, device=DEV)
        _fid().accumulate(mean, cov, real.to(DEV).float())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            s = kernel_timer.summary()
    finally:
        kernel_timer.enable(False)
    for name in ("knn_radius<f16>", "manifold_hits<f16>", "feature_stats_accum<f32>"):
        assert name in s and s[name]["total_ms"] > 0, (name, sorted(s))
