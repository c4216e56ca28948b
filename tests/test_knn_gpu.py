"""Fused Gram + row top-k kernel and the CKNNA sums (csrc/knn.hip) behind torch_utils/ops/knn_hip.py and
tools/evaluate_alignment/metrics.py on the GPU.

References: the fp64 Gram on the CPU with a stable descending sort (alignment_cases.topk64), the dense fp64
CKNNA formula (alignment_cases.dense_cknna64) and the reference's own values (tests/golden/
alignment_golden.npz). Tolerances (alignment_cases.py): a score within d 2^-24 of fp64, two scores swap only
within tol(d) = 2 d 2^-24, a CKNNA value within 4 d 2^-24."""
import functools
import importlib.util
import os

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import alignment_cases as ac
from conftest import PKG
from test_alignment_metrics import _vae, extractor_setup  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _metrics():
    path = os.path.join(PKG, "tools", "evaluate_alignment", "metrics.py")
    spec = importlib.util.spec_from_file_location("alignment_metrics_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _case(n, d, seed):
    """(a, b) normalised fp32 on the CPU. Computed once and shared; never modified."""
    return ac.make_features(n, d, seed)


@functools.lru_cache(maxsize=None)
def _ref(n, d, seed, which, k):
    """fp64 (idx, val, boundary gaps) of one feature set of a case."""
    f = _case(n, d, seed)[which]
    return ac.topk64(f, k) + (ac.boundary_gaps(f, k),)


def _knn():
    from torch_utils.ops import knn_hip
    return knn_hip


def _check_lists(f, idx, val, k, exclude_self=True, scale=1.0):
    """The tolerance rule on one (idx, val) against the fp64 scores of f (CPU fp32 features); nothing is excluded.
    `scale`: the largest product of two row norms (1 for normalised rows)."""
    n, d = f.shape
    s = ac.scores64(f, exclude_self)
    idx, val = idx.cpu().long(), val.cpu().double()
    assert idx.shape == val.shape == (n, k)
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    assert all(len(set(r)) == k for r in idx.tolist())                       # k distinct indices per row
    if exclude_self:
        assert not (idx == torch.arange(n)[:, None]).any()
    got = s.gather(1, idx)
    assert float((val - got).abs().max()) <= ac.val_tol(d) * scale
    assert (val[:, :-1] >= val[:, 1:]).all()                                  # descending
    same = val[:, :-1] == val[:, 1:]
    assert (idx[:, :-1][same] < idx[:, 1:][same]).all()                      # equal values by ascending index
    ri, rv = ac.topk64(f, k, exclude_self)
    clear = ac.boundary_gaps(f, k, exclude_self) > ac.tol(d) * scale
    assert torch.equal(idx.sort(dim=1).values[clear], ri.sort(dim=1).values[clear])
    assert (got.min(dim=1).values >= rv[:, -1] - ac.tol(d) * scale).all()
    return int((~clear).sum())


# ------------------------------------------------------------------ gap-safe cases

@pytest.mark.parametrize("case", ac.GAP_SAFE, ids=lambda c: ac.tag(*c))
def test_gap_safe_sets_values_and_cknna(case):
    n, d, k, seed = case
    a, b = _case(n, d, seed)
    lists = []
    for which, f in enumerate((a, b)):
        ri, rv, gaps = _ref(n, d, seed, which, k)
        assert float(gaps.min()) >= 10 * ac.tol(d)
        idx, val = _knn().gram_topk(f.to(DEV), k)
        assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.is_cuda
        assert torch.equal(idx.cpu().long().sort(dim=1).values, ri.sort(dim=1).values)
        err = float((val.cpu().double() - ac.scores64(f).gather(1, idx.cpu().long())).abs().max())
        print(f"set {which}: max |val - fp64| {err:.3e} (bound {ac.val_tol(d):.3e})")
        assert err <= ac.val_tol(d)
        assert _check_lists(f, idx, val, k) == 0
        lists.append((idx, val))
    got = _metrics().AlignmentMetrics.cknna(a.to(DEV), b.to(DEV), topk=k)
    gold = ac.golden_case(*case)
    print(f"cknna {got!r} golden {gold['cknna64']!r} diff {abs(got - gold['cknna64']):.3e} (bound {ac.cknna_tol(d):.3e})")
    assert abs(got - gold["cknna64"]) <= ac.cknna_tol(d)
    M = _metrics().AlignmentMetrics
    assert abs(M.mutual_knn(a.to(DEV), b.to(DEV), topk=k) - gold["mutual_knn"]) <= 1e-6
    assert abs(M.cycle_knn(a.to(DEV), b.to(DEV), topk=k) - gold["cycle_knn"]) <= 1e-6
    # the kernel's sums against the torch path's on the same lists
    t_hip = _knn().cknna_terms(lists[0][0], lists[0][1], lists[1][0], lists[1][1]).cpu()
    t_ref = _knn().cknna_terms_ref(lists[0][0].cpu(), lists[0][1].cpu(), lists[1][0].cpu(), lists[1][1].cpu())
    assert torch.allclose(t_hip, t_ref, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ ambiguous cases

@pytest.mark.parametrize("case,expect", list(zip(ac.AMBIGUOUS, (16, 3))), ids=lambda c: str(c))
def test_ambiguous_cases_follow_the_tolerance_rule(case, expect):
    n, d, k, seed = case
    a, b = _case(n, d, seed)
    ia, va = _knn().gram_topk(a.to(DEV), k)
    ib, vb = _knn().gram_topk(b.to(DEV), k)
    unclear = _check_lists(a, ia, va, k) + _check_lists(b, ib, vb, k)
    assert unclear == expect                                                  # the rows the case was chosen for
    got = _metrics().AlignmentMetrics.cknna(a.to(DEV), b.to(DEV), topk=k)
    dense = ac.dense_cknna64(a, b, ia, ib)
    print(f"cknna {got!r} dense fp64 on the op's lists {dense!r} diff {abs(got - dense):.3e}")
    assert abs(got - dense) <= ac.cknna_tol(d)


# ------------------------------------------------------------------ exact ties

@pytest.mark.parametrize("duplicate", [False, True])
def test_exact_ties_resolve_by_index(duplicate):
    g = torch.Generator().manual_seed(0)
    f = torch.randint(-3, 4, (150, 16), generator=g).float()                 # the Gram is exact in fp32
    if duplicate:
        f[90] = f[5]
    for k in (12, 64):
        ri, rv = ac.topk64(f, k)
        idx, val = _knn().gram_topk(f.to(DEV), k)
        assert torch.equal(idx.cpu().long(), ri) and torch.equal(val.cpu().double(), rv)
    if duplicate:                                                             # a copy of row i is a legal neighbour of i
        assert 90 in idx[5].tolist() and 5 in idx[90].tolist() and 5 not in idx[5].tolist()
    for splits in (2, 3):                                                     # ties across a split boundary too
        f2 = torch.cat([f, f, f])[:400]                                       # every row twice or three times
        ri, rv = ac.topk64(f2, 9)
        idx, val = _knn().gram_topk(f2.to(DEV), 9, splits=splits)
        assert torch.equal(idx.cpu().long(), ri) and torch.equal(val.cpu().double(), rv)


def test_torch_path_on_gpu_keeps_the_tie_rule():
    """The torch path on ROCm tensors (set_force_ref, and k past the kernel's 64): exact ties by ascending index,
    -0.0 == 0.0, element for element as the kernel and the fp64 stable sort give them."""
    g = torch.Generator().manual_seed(0)
    f = torch.randint(-3, 4, (150, 16), generator=g).float()
    f[90] = f[5]
    f[:, 0] = torch.where(torch.arange(150) % 2 == 0, torch.tensor(0.0), torch.tensor(-0.0))   # +-0 products
    z = torch.zeros(6, 4)
    z[:, 0] = torch.tensor([0.0, -0.0, 0.0, -0.0, 0.0, -0.0])                # every score is +0 or -0
    fd, zd = f.to(DEV), z.to(DEV)
    hip = _knn().gram_topk(fd, 12)
    ri65, rv65 = ac.topk64(f, 65)
    i65, v65 = _knn().gram_topk(fd, 65)                                       # k > 64: the torch path
    assert torch.equal(i65.cpu().long(), ri65) and torch.equal(v65.cpu().double(), rv65)
    zhip = _knn().gram_topk(zd, 3)[0]
    _knn().set_force_ref(True)
    try:
        ref = _knn().gram_topk(fd, 12)
        zref = _knn().gram_topk(zd, 3)[0]
    finally:
        _knn().set_force_ref(False)
    ri, rv = ac.topk64(f, 12)
    assert torch.equal(ref[0].cpu().long(), ri) and torch.equal(ref[1].cpu().double(), rv)
    assert torch.equal(ref[0], hip[0]) and torch.equal(ref[1], hip[1])
    expect = [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2], [0, 1, 2]]
    assert zref.tolist() == expect and zhip.tolist() == expect


# ------------------------------------------------------------------ edges

@pytest.mark.parametrize("D", [1, 5, 513])
@pytest.mark.parametrize("N", [4, 31, 33, 129])
def test_edge_sizes(N, D):
    g = torch.Generator().manual_seed(N * 1000 + D)
    f = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    fd = f.to(DEV)
    for k in (1, 2, 64, N - 1):
        if k > N - 1:
            continue
        idx, val = _knn().gram_topk(fd, k)
        _check_lists(f, idx, val, k)
        if D == 1:                                                            # scores are exactly +-1: pure tie rule
            ri, rv = ac.topk64(f, k)
            assert torch.equal(idx.cpu().long(), ri) and torch.equal(val.cpu().double(), rv)


def test_leading_dimension_and_include_self():
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(129, 47, generator=g)
    for c0, D in ((3, 33), (4, 32), (0, 40)):                                 # unaligned slice, aligned slice with ld > D
        f = torch.nn.functional.normalize(wide[:, c0:c0 + D], dim=-1)
        big = torch.zeros(129, 48)
        big[:, c0:c0 + D] = f
        view = big.to(DEV)[:, c0:c0 + D]
        assert view.stride(0) == 48 and not view.is_contiguous()
        idx, val = _knn().gram_topk(view, 7)
        _check_lists(f, idx, val, 7)
        i2, v2 = _knn().gram_topk(view.contiguous(), 7)
        assert torch.equal(idx, i2) and torch.equal(val, v2)
        idx, val = _knn().gram_topk(view, 7, exclude_self=False)
        _check_lists(f, idx, val, 7, exclude_self=False)
        assert torch.equal(idx[:, 0].cpu().long(), torch.arange(129))         # the diagonal comes first
    f = torch.randn(33, 20, generator=g) * 3.0                                # general rows: the bound scales
    idx, val = _knn().gram_topk(f.to(DEV), 33, exclude_self=False)
    _check_lists(f, idx, val, 33, exclude_self=False, scale=float(f.norm(dim=1).max()) ** 2)


# ------------------------------------------------------------------ determinism, memory, routing

@pytest.mark.parametrize("N,D", [(130, 32), (1000, 24)])
def test_splits_and_reruns_are_bit_identical(N, D):
    a, b = ac.make_features(N, D, 3)
    ad, bd = a.to(DEV), b.to(DEV)
    base = _knn().gram_topk(ad, 10, splits=1)
    chosen = set()
    for splits in (0, 2, 3, 7):
        chosen.add(_knn().gram_topk_workspace(N, 10, splits)[1])
        idx, val = _knn().gram_topk(ad, 10, splits=splits)
        assert torch.equal(idx, base[0]) and torch.equal(val, base[1])
    assert len(chosen) >= (3 if N == 1000 else 1)
    M = _metrics().AlignmentMetrics
    assert M.cknna(ad, bd, topk=10) == M.cknna(ad, bd, topk=10)
    t1 = _knn().cknna_terms(*_knn().gram_topk(ad, 10), *_knn().gram_topk(bd, 10))
    t2 = _knn().cknna_terms(*_knn().gram_topk(ad, 10), *_knn().gram_topk(bd, 10))
    assert torch.equal(t1, t2)


def test_no_score_matrix_in_memory():
    N, D, k = 4096, 64, 10
    g = torch.Generator().manual_seed(1)
    a = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1).to(DEV)
    b = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1).to(DEV)
    M = _metrics().AlignmentMetrics
    M.cknna(a[:256], b[:256], topk=k)                                         # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    value = M.cknna(a, b, topk=k)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"cknna {value!r}: peak rise {rise} bytes, N*N = {N * N}")
    assert rise < N * N                                                       # a quarter of one fp32 score matrix
    assert -1.0 < value < 1.0


class _Record(TorchDispatchMode):
    BAD = ("aten.mm", "aten.matmul", "aten.bmm", "aten.addmm", "aten.topk", "aten.sort", "aten.argsort",
           "aten.scatter")

    def __init__(self):
        super().__init__()
        self.hits = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if str(func).startswith(self.BAD):
            self.hits.append(str(func))
        return func(*args, **(kwargs or {}))


def test_routing():
    n, d, k, seed = ac.GAP_SAFE[1]
    a, b = _case(n, d, seed)
    ad, bd = a.to(DEV), b.to(DEV)
    M = _metrics().AlignmentMetrics
    with _Record() as rec:
        value = M.cknna(ad, bd, topk=k)
    assert rec.hits == [], rec.hits
    assert _knn().supported(ad, k) and not _knn().supported(ad, 65) and not _knn().supported(a, k)
    assert not _knn().supported(ad.double(), k) and not _knn().supported(ad, n)
    idx, _ = _knn().gram_topk(ad, k)
    sets = idx.cpu().long().sort(dim=1).values
    with _Record() as rec:
        i65, v65 = _knn().gram_topk(ad, 65)                                   # past the kernel's k: the torch path
    assert any(h.startswith("aten.sort") for h in rec.hits) and i65.shape == (n, 65) and i65.is_cuda
    assert torch.equal(i65[:, :k].cpu().long().sort(dim=1).values, sets)
    icpu, _ = _knn().gram_topk(a, k)                                          # CPU tensors: the torch path
    assert not icpu.is_cuda and torch.equal(icpu.long().sort(dim=1).values, sets)
    _knn().set_force_ref(True)
    try:
        with _Record() as rec:
            forced = M.cknna(ad, bd, topk=k)
        assert any(h.startswith("aten.sort") for h in rec.hits)
    finally:
        _knn().set_force_ref(False)
    assert abs(forced - value) <= ac.cknna_tol(d)


def test_extractor_on_gpu_matches_cpu(extractor_setup):  # noqa: F811
    """The extractor's clean mode on cuda:0 against the CPU run, same posterior noise (CPU RNG, same seed):
    features within 5e-2 relative L2, the bound tests/test_tools.py uses for the latent prefetch tools (the
    SigLIP2 tower runs under bf16 autocast on the GPU, fp32 on the CPU)."""
    s, ext = extractor_setup, extractor_setup["ext"]
    got = {}
    for dev in ("cpu", "cuda:0"):
        G = _vae(s, dev)
        out = s["root"] / f"feats_{dev.replace(':', '')}"
        torch.manual_seed(23)
        files = ext.extract_features(G, str(s["data"]), str(out), "tiny", "clean", 64, 2, s["common"].Rank(dev),
                                     log=lambda *a: None)
        got[dev] = torch.load(files[0], weights_only=True)
    c, g = got["cpu"], got["cuda:0"]
    assert c["names"] == g["names"] == s["stems"] and c["transformations"] == g["transformations"]
    assert not g["features"].is_cuda and g["features"].shape == c["features"].shape
    rel = float((g["features"].double() - c["features"].double()).norm() / c["features"].double().norm())
    print(f"relative L2 {rel:.3e}")
    assert rel < 5e-2
