"""Running Frechet-distance statistics as a HIP kernel (csrc/fidstats.hip; reference
metrics/metric_utils.py:109-124 `FeatureStats.append`: every batch copied to the host and multiplied there as
`x64.T @ x64` in numpy). Reached through metrics/metric_utils.py `FeatureStats.append_torch`.

accumulate(raw_mean, raw_cov, x): in place raw_mean[D] += sum_r x_r and raw_cov[D, D] += X^T X, fp64, with x
widened to fp64 before the product. fp32 / fp16 ROCm batches run on the fp64 MFMA kernel (no host sync, one
summation order per element: two runs agree bitwise); CPU tensors, other dtypes and set_force_ref(True) take
the torch fp64 path."""
import torch

from .. import custom_ops
from . import kernel_timer

_FORCE_REF = False
_TNAME = {torch.float32: "f32", torch.float16: "f16"}


def set_force_ref(flag: bool):
    """Route every call to the torch path (to compare the two paths on the GPU)."""
    global _FORCE_REF
    _FORCE_REF = bool(flag)


def force_ref() -> bool:
    return _FORCE_REF


def supported(raw_mean, raw_cov, x):
    return x.is_cuda and x.dtype in _TNAME and raw_mean.is_cuda and raw_cov.is_cuda


def accumulate_ref(raw_mean, raw_cov, x):
    """The torch path: the reference's two lines in fp64 on x's device."""
    x64 = x.to(torch.float64)
    raw_mean += x64.sum(dim=0)
    raw_cov += x64.T @ x64


def accumulate(raw_mean, raw_cov, x):
    """raw_mean [D] and raw_cov [D, D] (fp64, contiguous, on x's device) += the sums of batch x [n, D]."""
    if x.dim() != 2:
        raise ValueError(f"x must be [n, D], not {tuple(x.shape)}")
    n, D = x.shape
    if D < 1 or tuple(raw_mean.shape) != (D,) or tuple(raw_cov.shape) != (D, D):
        raise ValueError(f"raw_mean {tuple(raw_mean.shape)} / raw_cov {tuple(raw_cov.shape)} do not fit x {tuple(x.shape)}")
    if raw_mean.dtype != torch.float64 or raw_cov.dtype != torch.float64:
        raise ValueError("raw_mean and raw_cov must be float64")
    if not (raw_mean.is_contiguous() and raw_cov.is_contiguous()):
        raise ValueError("raw_mean and raw_cov must be contiguous (they are updated in place)")
    if raw_mean.device != x.device or raw_cov.device != x.device:
        raise ValueError("raw_mean, raw_cov and x must share one device")
    if n == 0:
        return
    if _FORCE_REF or not supported(raw_mean, raw_cov, x):
        return accumulate_ref(raw_mean, raw_cov, x)
    if x.stride(1) != 1 or x.stride(0) < D:
        x = x.contiguous()
    lib = custom_ops.get_native()
    esize = x.element_size()
    with kernel_timer.region(f"feature_stats_accum<{_TNAME[x.dtype]}>", n * D * esize + 16 * D * D, 2 * n * D * D,
                             bound="hbm"):
        custom_ops.check(lib.vfm_feature_stats_accum(x.data_ptr(), custom_ops.dtype_code(x), x.stride(0), n, D,
                                                     raw_mean.data_ptr(), raw_cov.data_ptr(),
                                                     custom_ops.stream_ptr()), "vfm_feature_stats_accum")
