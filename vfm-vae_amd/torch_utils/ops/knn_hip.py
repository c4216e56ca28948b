"""Nearest neighbours by inner product and the CKNNA sums as HIP kernels (csrc/knn.hip; reference
tools/evaluate_alignment/metrics.py:191-260 and :283-296: dense N x N Gram matrices, torch.topk / argsort,
scattered N x N masks and an N x N . N x N torch.mm). Reached through tools/evaluate_alignment/metrics.py.

gram_topk: for every row of `feats` the k largest inner products with the other rows, as (idx int32 [N, k],
val [N, k]), descending value, EQUAL VALUES BY ASCENDING INDEX (-0.0 == 0.0) -- a definite rule on both
paths (torch.topk leaves ties unspecified). fp32 ROCm features with k <= 64 run on the fused Gram + top-k
kernel (exact fp32 products on the fp32 MFMA, no score matrix in memory); CPU tensors, other dtypes, larger
k and set_force_ref(True) take the torch path: row chunks of the Gram (rows x N at a time, never N x N) and
a stable descending sort. Non-finite features are not supported (a NaN score has no place in the order);
callers check once (the alignment tool does on load).

cknna_terms: the nine fp64 sums of include/vfmvae.h `vfm_cknna_terms` from two neighbour lists."""
import ctypes

import torch

from .. import custom_ops
from . import kernel_timer

MAX_K = 64                 # csrc/knn.hip MAXK
_FORCE_REF = False
_CHUNK_ELEMS = 1 << 24     # score elements of one row chunk of the torch path


def set_force_ref(flag: bool):
    """Route every call to the torch path (to compare the two paths on the GPU)."""
    global _FORCE_REF
    _FORCE_REF = bool(flag)


def force_ref() -> bool:
    return _FORCE_REF


def supported(feats, k, exclude_self=True):
    """The inputs the kernel covers: 2-d fp32 ROCm features, 1 <= k <= min(64, N - exclude_self), N < 2^31."""
    if not (torch.is_tensor(feats) and feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 2):
        return False
    N, D = feats.shape
    return D >= 1 and N < 2 ** 31 and 1 <= k <= MAX_K and k <= N - int(bool(exclude_self))


def _check_k(feats, k, exclude_self):
    if feats.dim() != 2:
        raise ValueError(f"feats must be [N, D], not {tuple(feats.shape)}")
    N = feats.shape[0]
    if not 1 <= k <= N - int(bool(exclude_self)):
        raise ValueError(f"k = {k} outside 1 .. {N - int(bool(exclude_self))} for N = {N}")


def gram_topk_ref(feats, k, exclude_self=True):
    """The torch path: row chunks of feats @ feats.T, the diagonal at -inf, stable descending sort."""
    N = feats.shape[0]
    rows = max(1, min(N, _CHUNK_ELEMS // max(N, 1)))
    idx = torch.empty([N, k], dtype=torch.int32, device=feats.device)
    val = torch.empty([N, k], dtype=feats.dtype, device=feats.device)
    for r0 in range(0, N, rows):
        s = feats[r0:r0 + rows] @ feats.T + 0.0          # -0.0 -> +0.0: a sort by bit pattern sees them equal too
        if exclude_self:
            ar = torch.arange(s.shape[0], device=feats.device)
            s[ar, ar + r0] = float("-inf")
        v, i = torch.sort(s, dim=1, descending=True, stable=True)
        idx[r0:r0 + rows] = i[:, :k]
        val[r0:r0 + rows] = v[:, :k]
    return idx, val


def gram_topk_workspace(N, k, splits=0):
    """(workspace bytes, split count) of vfm_gram_topk for these sizes (host query)."""
    chosen = ctypes.c_int(0)
    nbytes = custom_ops.get_native().vfm_gram_topk_ws(N, k, splits, ctypes.byref(chosen))
    if nbytes < 0:
        raise custom_ops.NativeError(f"vfm_gram_topk_ws failed with code {nbytes}")
    return nbytes, chosen.value


def gram_topk(feats, k, exclude_self=True, splits=0):
    """(idx int32 [N, k], val [N, k]) of the k largest <f_i, f_j> per row i, j != i when exclude_self."""
    k = int(k)
    _check_k(feats, k, exclude_self)
    if _FORCE_REF or not supported(feats, k, exclude_self):
        return gram_topk_ref(feats, k, exclude_self)
    if feats.stride(1) != 1 or feats.stride(0) < feats.shape[1]:
        feats = feats.contiguous()
    N, D = feats.shape
    lib = custom_ops.get_native()
    nbytes, _ = gram_topk_workspace(N, k, splits)
    ws = torch.empty([nbytes], dtype=torch.uint8, device=feats.device) if nbytes else None
    idx = torch.empty([N, k], dtype=torch.int32, device=feats.device)
    val = torch.empty([N, k], dtype=torch.float32, device=feats.device)
    with kernel_timer.region("gram_topk<f32>", 4 * N * D, 2 * N * N * D, bound="mfma"):
        custom_ops.check(lib.vfm_gram_topk(feats.data_ptr(), feats.stride(0), N, D, k, int(bool(exclude_self)),
                                           int(splits), idx.data_ptr(), val.data_ptr(), custom_ops.ptr(ws),
                                           custom_ops.stream_ptr()), "vfm_gram_topk")
    return idx, val


def in_other(ia, ib, rows=None):
    """[N, k] bool: entry p of row i's list a is also in row i's list b (`rows` lists at a time as [rows, k, k])."""
    if rows is None:
        rows = max(1, (1 << 22) // (ia.shape[1] * ib.shape[1]))
    out = torch.empty(ia.shape, dtype=torch.bool, device=ia.device)
    for r0 in range(0, ia.shape[0], rows):
        out[r0:r0 + rows] = (ia[r0:r0 + rows, :, None] == ib[r0:r0 + rows, None, :]).any(-1)
    return out


def _hsic_terms_ref(ia, a, ib, b, rows):
    """(cross, sum A . sum B, product) for A, B given as row lists (indices, values with the mask applied)."""
    N = ia.shape[0]
    prod = (a * b.sum(1)[ia]).sum()
    cross = a.new_zeros([])
    for r0 in range(0, N, rows):
        j = ia[r0:r0 + rows]                                              # [c, k]
        me = torch.arange(r0, r0 + j.shape[0], device=ia.device)[:, None, None]
        bji = (b[j] * (ib[j] == me)).sum(-1)                               # B_ji from row j's list
        cross = cross + (a[r0:r0 + rows] * bji).sum()
    return torch.stack([cross, a.sum() * b.sum(), prod])


def cknna_terms_ref(idxK, valK, idxL, valL):
    """The torch path of cknna_terms: [N, k] tensor ops in fp64, row-chunked."""
    iK, iL = idxK.long(), idxL.long()
    vK, vL = valK.double(), valL.double()
    k = iK.shape[1]
    rows = max(1, (1 << 22) // (k * k))
    mK, mL = in_other(iK, iL, rows), in_other(iL, iK, rows)
    return torch.cat([_hsic_terms_ref(iK, vK * mK, iL, vL * mL, rows),
                      _hsic_terms_ref(iK, vK, iK, vK, rows),
                      _hsic_terms_ref(iL, vL, iL, vL, rows)])


def cknna_terms(idxK, valK, idxL, valL):
    """fp64 [9]: (cross, sum A . sum B, product) of hsic_unbiased(M o K, M o L), (M_K o K, M_K o K) and
    (M_L o L, M_L o L), M(i) the intersection of row i's two lists (`vfm_cknna_terms`). The lists must not hold
    their own row (gram_topk with exclude_self=True): hsic_unbiased zeroes the diagonal, and every list entry is
    taken as off-diagonal here."""
    if not (idxK.shape == valK.shape == idxL.shape == valL.shape and idxK.dim() == 2):
        raise ValueError("the four lists must share one [N, k] shape")
    N, k = idxK.shape
    ok = all(t.is_cuda for t in (idxK, valK, idxL, valL)) and valK.dtype == valL.dtype == torch.float32 \
        and idxK.dtype == idxL.dtype == torch.int32 and 1 <= k <= MAX_K and N < 2 ** 31
    if _FORCE_REF or not ok:
        return cknna_terms_ref(idxK, valK, idxL, valL)
    lib = custom_ops.get_native()
    idxK, valK, idxL, valL = (t.contiguous() for t in (idxK, valK, idxL, valL))
    nbytes = lib.vfm_cknna_terms_ws(N)
    if nbytes < 0:
        raise custom_ops.NativeError(f"vfm_cknna_terms_ws failed with code {nbytes}")
    ws = torch.empty([nbytes], dtype=torch.uint8, device=idxK.device)
    out = torch.empty([9], dtype=torch.float64, device=idxK.device)
    with kernel_timer.region("cknna_terms<f32>", 16 * N * k):
        custom_ops.check(lib.vfm_cknna_terms(idxK.data_ptr(), valK.data_ptr(), idxL.data_ptr(), valL.data_ptr(), N, k,
                                             out.data_ptr(), ws.data_ptr(), custom_ops.stream_ptr()),
                         "vfm_cknna_terms")
    return out
