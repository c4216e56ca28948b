"""F.interpolate (bilinear / bicubic, with or without antialias) with a run-to-run reproducible backward.

torch's GPU backward kernels of these modes scatter every output gradient into the input plane with atomic adds
(`upsample_*2d[_aa]_backward_out_cuda`, which torch itself lists as nondeterministic): an input pixel that receives
more than two contributions gets them in an order that changes from run to run, so the gradient differs at
rounding level between two runs of the same step, and Adam (beta1 = 0) turns that into parameter differences that
grow with every step. The forward pass here is F.interpolate itself, unchanged. The backward applies the same
linear map's adjoint as a gather: the resize is separable, y = A_h x A_w^T, with the 1-D matrices read off
F.interpolate once per (sizes, mode) by resizing an identity pattern; each input column then sums its few
contributing outputs in a fixed order (dx = A_h^T dy A_w, one pass per axis).
"""
import functools

import torch
import torch.nn.functional as F

_MODES = ("bilinear", "bicubic")


@functools.lru_cache(maxsize=None)
def _axis_taps(n_in, n_out, mode, antialias, scale_factor):
    """(J [n_in, K] int64, W [n_in, K] float32) on the CPU: input index i receives sum_k W[i, k] * dy[J[i, k]]
    along the axis (K = the largest number of outputs one input contributes to; padded with weight 0)."""
    eye = torch.eye(n_in, dtype=torch.float64)
    if scale_factor is None:
        x = eye.view(1, n_in, 1, n_in).expand(1, n_in, 2, n_in).contiguous()       # x[0, c, h, w] = [c == w]
        y = F.interpolate(x, size=(2, n_out), mode=mode, align_corners=False, antialias=antialias)
    else:
        x = eye.view(1, n_in, 1, n_in).expand(1, n_in, n_in, n_in).contiguous()
        y = F.interpolate(x, scale_factor=scale_factor, mode=mode, align_corners=False, antialias=antialias)
    a = y[0, :, 0, :].t().contiguous()                      # A[j, c]: output j's weight on input c
    assert a.shape[1] == n_in and (scale_factor is not None or a.shape[0] == n_out)
    nz = a != 0
    k = max(1, int(nz.sum(0).max()))
    idx = torch.zeros(n_in, k, dtype=torch.int64)
    wts = torch.zeros(n_in, k, dtype=torch.float32)
    for i in range(n_in):
        js = torch.nonzero(nz[:, i]).flatten()
        idx[i, :len(js)] = js
        wts[i, :len(js)] = a[js, i].float()
    return idx, wts, a.shape[0]


@functools.lru_cache(maxsize=None)
def _device_taps(n_in, n_out, mode, antialias, scale_factor, device):
    idx, wts, n = _axis_taps(n_in, n_out, mode, antialias, scale_factor)
    return idx.to(device), wts.to(device), n


def _adjoint_last(dy, idx, wts):
    """dy [..., n_out] -> [..., n_in]: fixed-order sum of each input's contributing outputs."""
    return (dy[..., idx] * wts).sum(-1)


class _Resize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, scale_factor, mode, antialias):
        y = F.interpolate(x, size=size, scale_factor=scale_factor, mode=mode, align_corners=False, antialias=antialias)
        ctx.cfg = (tuple(x.shape[-2:]), tuple(y.shape[-2:]), scale_factor, mode, antialias)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (hi, wi), (ho, wo), sf, mode, aa = ctx.cfg
        dev = str(dy.device)
        jw, ww, _ = _device_taps(wi, wo, mode, aa, sf, dev)
        jh, wh, _ = _device_taps(hi, ho, mode, aa, sf, dev)
        t = _adjoint_last(dy.float(), jw, ww)                                   # [..., ho, wi]
        dx = _adjoint_last(t.transpose(-1, -2), jh, wh).transpose(-1, -2)       # [..., hi, wi]
        return dx.contiguous().to(dy.dtype), None, None, None, None


def interpolate(x, size=None, scale_factor=None, mode="bilinear", align_corners=False, antialias=False):
    """F.interpolate for 4-D input; a reproducible backward for the separable modes when a gradient is needed."""
    if (mode not in _MODES or align_corners or x.dim() != 4 or not x.requires_grad or not torch.is_grad_enabled()
            or isinstance(scale_factor, (tuple, list))):
        kw = dict(align_corners=align_corners) if mode in _MODES else {}
        if antialias:
            kw["antialias"] = True
        return F.interpolate(x, size=size, scale_factor=scale_factor, mode=mode, **kw)
    if isinstance(size, (tuple, list)):
        size = tuple(int(s) for s in size)
    sf = None if scale_factor is None else float(scale_factor)
    return _Resize.apply(x, size, sf, mode, bool(antialias))
