"""k-th neighbour radii and manifold membership by Euclidean distance as HIP kernels (csrc/prknn.hip;
reference metrics/precision_recall.py:21-63: 10 000 x 10 000 torch.cdist blocks copied to the host,
`kthvalue` and `(dist <= kth).any` there). Reached through metrics/precision_recall.py.

knn_radius(feats, k): fp16 [N], the (k + 1)-th smallest distance of every row to all N rows, itself included
(`dist.float().kthvalue(k + 1).values.half()`).
manifold_hits(probes, manifold, radii): (hits bool [P], mean fp32 scalar tensor): row i hits iff some j has
dist(i, j) <= radii[j]; the mean stays on the device.

fp16 ROCm features with k + 1 <= 64 run on the fused distance kernels (fp16 MFMA, fp32 accumulation, no
distance matrix in memory). CPU tensors, other dtypes, larger k and set_force_ref(True) take the torch path,
the reference arithmetic in row chunks (rows x N at a time, never N x N): torch.cdist on .float(),
kthvalue(k + 1), .half(), <=."""
import ctypes

import torch

from .. import custom_ops
from . import kernel_timer

MAX_K1 = 64                # csrc/prknn.hip MAXK1: k + 1 entries per row in LDS
_FORCE_REF = False
_CHUNK_ELEMS = 1 << 24     # distance elements of one row chunk of the torch path


def set_force_ref(flag: bool):
    """Route every call to the torch path (to compare the two paths on the GPU)."""
    global _FORCE_REF
    _FORCE_REF = bool(flag)


def force_ref() -> bool:
    return _FORCE_REF


def _fused(*tensors):
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float16 for t in tensors) and not _FORCE_REF


def _check_feats(name, t):
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError(f"{name} must be [N, D] with D >= 1, not {tuple(t.shape)}")
    if t.shape[0] >= 2 ** 31:
        raise ValueError(f"{name} has {t.shape[0]} rows; the limit is 2^31 - 1")


def _rows(N):
    return max(1, _CHUNK_ELEMS // max(N, 1))


def _rowmajor(t):
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def knn_radius_ref(feats, k, rows=None):
    """The torch path of knn_radius."""
    N = feats.shape[0]
    r_lo, r_hi = (0, N) if rows is None else rows
    cols = feats.unsqueeze(0).float()
    out = []
    for r0 in range(r_lo, r_hi, _rows(N)):
        dist = torch.cdist(feats[r0:min(r0 + _rows(N), r_hi)].unsqueeze(0).float(), cols)[0]
        out.append(dist.to(torch.float32).kthvalue(k + 1).values.to(torch.float16))
    return torch.cat(out)


def manifold_hits_ref(probes, manifold, radii):
    """The torch path of manifold_hits."""
    P, N = probes.shape[0], manifold.shape[0]
    cols = manifold.unsqueeze(0).float()
    out = []
    for r0 in range(0, P, _rows(N)):
        dist = torch.cdist(probes[r0:r0 + _rows(N)].unsqueeze(0).float(), cols)[0]
        out.append((dist <= radii).any(dim=1))
    hits = torch.cat(out)
    return hits, hits.to(torch.float32).mean()


def _ws(fn, name, *sizes, splits=0):
    chosen = ctypes.c_int(0)
    nbytes = fn(*sizes, int(splits), ctypes.byref(chosen))
    if nbytes < 0:
        raise custom_ops.NativeError(f"{name} failed with code {nbytes}")
    return nbytes, chosen.value


def knn_radius(feats, k, splits=0, rows=None):
    """fp16 [N]: the (k + 1)-th smallest Euclidean distance from each row of feats [N, D] to all N rows; with
    rows = (r0, r1) only for rows r0 .. r1 - 1 (a rank's slice)."""
    k = int(k)
    _check_feats("feats", feats)
    N, D = feats.shape
    if k < 0 or k + 1 > N:
        raise ValueError(f"k + 1 = {k + 1} neighbours asked of N = {N} rows")
    r0, r1 = (0, N) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 <= r1 <= N:
        raise ValueError(f"rows {rows} outside 0 .. {N}")
    if r0 == r1:
        return torch.empty([0], dtype=torch.float16, device=feats.device)
    if not _fused(feats) or k + 1 > MAX_K1:
        return knn_radius_ref(feats, k, (r0, r1))
    feats = _rowmajor(feats)
    lib = custom_ops.get_native()
    nbytes, _ = _ws(lib.vfm_knn_radius_ws, "vfm_knn_radius_ws", N, k, r1 - r0, splits=splits)
    ws = torch.empty([nbytes], dtype=torch.uint8, device=feats.device)
    radii = torch.empty([r1 - r0], dtype=torch.float16, device=feats.device)
    with kernel_timer.region("knn_radius<f16>", 2 * N * D, 2 * (r1 - r0) * N * D, bound="mfma"):
        custom_ops.check(lib.vfm_knn_radius(feats.data_ptr(), feats.stride(0), N, D, k, r0, r1 - r0, int(splits),
                                            radii.data_ptr(), ws.data_ptr(), custom_ops.stream_ptr()),
                         "vfm_knn_radius")
    return radii


def manifold_hits(probes, manifold, radii, splits=0):
    """(hits bool [P], mean of hits as an fp32 scalar tensor on the device)."""
    _check_feats("probes", probes)
    _check_feats("manifold", manifold)
    P, D = probes.shape
    N = manifold.shape[0]
    if manifold.shape[1] != D or tuple(radii.shape) != (N,) or P < 1 or N < 1:
        raise ValueError(f"probes {tuple(probes.shape)}, manifold {tuple(manifold.shape)} and radii "
                         f"{tuple(radii.shape)} do not fit")
    if not _fused(probes, manifold, radii):
        return manifold_hits_ref(probes, manifold, radii)
    probes, manifold, radii = _rowmajor(probes), _rowmajor(manifold), radii.contiguous()
    lib = custom_ops.get_native()
    nbytes, _ = _ws(lib.vfm_manifold_hits_ws, "vfm_manifold_hits_ws", P, N, splits=splits)
    ws = torch.empty([nbytes], dtype=torch.uint8, device=probes.device)
    hits = torch.empty([P], dtype=torch.uint8, device=probes.device)
    mean = torch.empty([], dtype=torch.float32, device=probes.device)
    with kernel_timer.region("manifold_hits<f16>", 2 * (P + N) * D, 2 * P * N * D, bound="mfma"):
        custom_ops.check(lib.vfm_manifold_hits(probes.data_ptr(), probes.stride(0), P, manifold.data_ptr(),
                                               manifold.stride(0), N, D, radii.data_ptr(), int(splits), hits.data_ptr(),
                                               mean.data_ptr(), ws.data_ptr(), custom_ops.stream_ptr()),
                         "vfm_manifold_hits")
    return hits.view(torch.bool), mean
