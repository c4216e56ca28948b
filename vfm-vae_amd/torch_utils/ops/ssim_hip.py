"""Gaussian SSIM loss and its gradient as HIP kernels (csrc/ssim.hip; reference training/loss.py:150-152,
257-260: torchmetrics' StructuralSimilarityIndexMeasure on clamped images). Reached through
training.loss.SSIM for fp32 ROCm images with the 11-tap window: two launches forward (tile kernel and
fixed-order finish), one backward per input that needs a gradient, the clamp fused in, nothing saved
between them but the two images."""
import ctypes
import functools

import torch

from .. import custom_ops
from . import kernel_timer

_lib = custom_ops.get_native()

KERNEL_SIZE = 11
TILE_H, TILE_W = 16, 32       # the kernels' tile (csrc/ssim.hip TH, TW): map tile forward, image tile backward


@functools.lru_cache(maxsize=None)
def gaussian_taps(size, sigma):
    """training.loss._gaussian_window in fp64, rounded to fp32, as the host array the launchers take."""
    x = torch.arange(size, dtype=torch.float64) - (size - 1) / 2
    g = torch.exp(-(x / sigma) ** 2 / 2)
    g = (g / g.sum()).float()
    return (ctypes.c_float * size)(*g.tolist())


def _clamp_args(clamp):
    return (0.0, 0.0, 0) if clamp is None else (float(clamp[0]), float(clamp[1]), 1)


class _SSIM(custom_ops.FastFunction):
    @staticmethod
    def forward(ctx, preds, target, taps, c1, c2, clamp):
        preds, target = preds.contiguous(), target.contiguous()
        B, C, H, W = preds.shape
        nparts = _lib.vfm_ssim_fwd_partials(B, C, H, W)
        if nparts <= 0:
            raise custom_ops.NativeError(f"vfm_ssim_fwd_partials failed with code {nparts}")
        partials = torch.empty([nparts], dtype=torch.float32, device=preds.device)
        out = torch.empty([], dtype=torch.float32, device=preds.device)
        lo, hi, on = _clamp_args(clamp)
        with kernel_timer.region("ssim_fwd<f32>", 4 * 2 * preds.numel()):
            custom_ops.check(_lib.vfm_ssim_fwd(preds.data_ptr(), target.data_ptr(), partials.data_ptr(), out.data_ptr(),
                                               taps, len(taps), c1, c2, lo, hi, on, B, C, H, W,
                                               custom_ops.stream_ptr()), "vfm_ssim_fwd")
        ctx.save_for_backward(preds, target)
        ctx.args = (taps, c1, c2, clamp)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        preds, target = ctx.saved_tensors
        taps, c1, c2, clamp = ctx.args
        B, C, H, W = preds.shape
        lo, hi, on = _clamp_args(clamp)
        dout = dout.float().contiguous()
        grads = [None, None]
        for k, (a, b) in enumerate(((preds, target), (target, preds))):
            if not ctx.needs_input_grad[k]:
                continue
            da = torch.empty_like(a)
            # S is symmetric in its two images: the gradient to target is the same kernel, roles swapped
            with kernel_timer.region("ssim_bwd<f32>", 4 * 3 * a.numel()):
                custom_ops.check(_lib.vfm_ssim_bwd(a.data_ptr(), b.data_ptr(), dout.data_ptr(), da.data_ptr(), taps,
                                                   len(taps), c1, c2, lo, hi, on, B, C, H, W,
                                                   custom_ops.stream_ptr()), "vfm_ssim_bwd")
            grads[k] = da
        return grads[0], grads[1], None, None, None, None


def supported(preds, target, kernel_size):
    """The shapes and types the kernels cover: equal-shape 4-d fp32 ROCm images at least one window large."""
    return (preds.is_cuda and target.is_cuda and preds.dtype == target.dtype == torch.float32 and preds.dim() == 4
            and preds.shape == target.shape and kernel_size == KERNEL_SIZE
            and min(preds.shape[-2:]) >= kernel_size and preds.numel() > 0)


def ssim(preds, target, kernel_size, sigma, c1, c2, clamp=None):
    """mean SSIM of clamp(preds) and clamp(target) (clamp: None or (lo, hi)); 0-dim fp32."""
    return _SSIM.apply(preds, target, gaussian_taps(kernel_size, float(sigma)), float(c1), float(c2),
                       None if clamp is None else (float(clamp[0]), float(clamp[1])))
