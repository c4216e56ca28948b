"""Shared inputs and fp64 restatements for the alignment-metric tests (test_alignment_metrics.py,
test_knn_gpu.py) and tests/golden/make_golden_alignment.py.

Tolerance, derived once: for unit-norm rows an fp32 dot product of length d, in any accumulation order, is
within d 2^-24 of the true value (the standard bound sum |a_i b_i| d u with Cauchy-Schwarz, u = 2^-24). Two
compared scores can therefore swap only when they are closer than tol(d) = 2 d 2^-24. A CKNNA value is a ratio
of sums of products of two such scores, each product within 2 d 2^-24 of the true one to first order, and the
ratio's normalisation keeps the bound: 4 d 2^-24 with the factor two of the quotient."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alignment_golden.npz")

# (n, d, k, seed)
GAP_SAFE = [(67, 48, 10, 2), (200, 32, 10, 0), (130, 96, 2, 0), (257, 33, 10, 13)]
AMBIGUOUS = [(333, 512, 10, 0), (1000, 64, 10, 0)]


def tag(n, d, k, seed):
    return f"n{n}_d{d}_k{k}_s{seed}"


def val_tol(d):
    return d * 2.0 ** -24


def tol(d):
    return 2.0 * d * 2.0 ** -24


def cknna_tol(d):
    return 4.0 * d * 2.0 ** -24


def make_features(n, d, seed):
    """Two correlated feature sets, normalised fp32 [n, d]; everything drawn on the CPU generator, in this order."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, d, dtype=torch.float64, generator=g)
    w = torch.randn(d, d, dtype=torch.float64, generator=g)
    e = torch.randn(n, d, dtype=torch.float64, generator=g)
    b = 0.6 * a @ w / math.sqrt(d) + 0.8 * e
    return F.normalize(a.float(), dim=-1), F.normalize(b.float(), dim=-1)


def make_raw_pair():
    """Raw (unnormalised) fp32 feature pair with a few large outliers, as an extractor would save it."""
    g = torch.Generator().manual_seed(7)
    r1 = torch.randn(40, 24, generator=g) * 3.0 + 0.5
    r2 = torch.randn(40, 16, generator=g)
    r1[3, 5], r1[17, 0], r1[30, 23] = 250.0, -400.0, 90.0
    r2[0, 0], r2[39, 15] = 75.0, -60.0
    return r1, r2


def scores64(f, exclude_self=True):
    s = f.double().cpu() @ f.double().cpu().T
    if exclude_self:
        s.fill_diagonal_(float("-inf"))
    return s


def topk64(f, k, exclude_self=True):
    """(idx, val) of the fp64 scores by stable descending sort: equal values by ascending index."""
    v, i = torch.sort(scores64(f, exclude_self), dim=1, descending=True, stable=True)
    return i[:, :k], v[:, :k]


def boundary_gaps(f, k, exclude_self=True):
    """Per row: k-th minus (k+1)-th fp64 score (inf when there is no (k+1)-th)."""
    v = torch.sort(scores64(f, exclude_self), dim=1, descending=True).values
    if k >= v.shape[1] or (exclude_self and k >= v.shape[1] - 1):
        return torch.full([v.shape[0]], float("inf"), dtype=torch.float64)
    return v[:, k - 1] - v[:, k]


def min_boundary_gap(f, k):
    return float(boundary_gaps(f, k).min())


def hsic_unbiased64(K, L):
    """Song et al. 2012 eq. 5 on dense fp64 matrices (the formula the reference's hsic_unbiased states)."""
    m = K.shape[0]
    Kt, Lt = K.clone().fill_diagonal_(0), L.clone().fill_diagonal_(0)
    h = (Kt * Lt.T).sum() + Kt.sum() * Lt.sum() / ((m - 1) * (m - 2)) - 2 * (Kt @ Lt).sum() / (m - 2)
    return h / (m * (m - 3))


def dense_cknna64(a, b, idx_K, idx_L):
    """The dense formulation in fp64 with masks built from the given neighbour lists."""
    K, L = a.double().cpu() @ a.double().cpu().T, b.double().cpu() @ b.double().cpu().T
    n = K.shape[0]
    mK = torch.zeros(n, n, dtype=torch.float64).scatter_(1, idx_K.long().cpu(), 1.0)
    mL = torch.zeros(n, n, dtype=torch.float64).scatter_(1, idx_L.long().cpu(), 1.0)
    m = mK * mL
    kl = hsic_unbiased64(m * K, m * L)
    kk = hsic_unbiased64(mK * K, mK * K)
    ll = hsic_unbiased64(mL * L, mL * L)
    return float(kl) / (float(torch.sqrt(kk * ll)) + 1e-6)


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def golden_case(n, d, k, seed):
    g, t = golden(), tag(n, d, k, seed)
    return {key.split("/", 1)[1]: (torch.from_numpy(v) if v.ndim else float(v)) for key, v in g.items()
            if key.startswith(t + "/")}
