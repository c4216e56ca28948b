"""gfx950 kernels of the frozen Qwen2.5-VL vision tower (csrc/qwen.hip, C ABI in include/vfmvae.h).

Varlen RoPE attention (head dim 80, block-diagonal over a device-resident cu_seqlens), RMSNorm rows on a
bf16 / fp32 stream (plain and fused with the residual add), SwiGLU rows over the padded gate | up
projection, and the patch gather into window order. Forward only: the tower is frozen and runs under
no_grad (reference networks/utils/vfms/qwen_utils.py:203). Loading the library raises if it is missing
(no silent fallback on ROCm tensors); the torch formulations live in vit_ops.
"""
import os

import torch

from .. import custom_ops
from . import kernel_timer

_lib = custom_ops.get_native()
HEAD_DIM = 80
_DN = {torch.float32: "f32", torch.bfloat16: "bf16"}


def _no_grad(name, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError(f"qwen_hip.{name} is forward-only (frozen tower under no_grad)")


def attention_supported(qkv, head_dim):
    return qkv.is_cuda and qkv.dtype == torch.bfloat16 and head_dim == HEAD_DIM


def attention_waves(max_seqlen):
    """Waves per workgroup the library picks for this hint (csrc/qwen.hip): 2 where no segment is longer than
    one 64-key tile, 8 from 512 keys, else 4; VFM_QWEN_ATTN_WAVES=1|2|4|8 forces one (A/B, read by the library
    at every call)."""
    forced = os.environ.get("VFM_QWEN_ATTN_WAVES", "")
    if forced in ("1", "2", "4", "8"):
        return int(forced)
    if max_seqlen <= 0:
        return 4
    return 2 if max_seqlen <= 64 else 8 if max_seqlen >= 512 else 4


def rope_attention_varlen(qkv, cos, sin, cu_seqlens, heads, max_seqlen=0, out=None):
    """qkv: bf16 [T, 3 * heads * 80] (q | k | v, heads contiguous inside each); cos / sin: fp32 [T, 80];
    cu_seqlens: int32 [S + 1] on the device -> o bf16 [T, heads * 80]. max_seqlen: host hint (0: unknown)."""
    _no_grad("rope_attention_varlen", qkv)
    T, D3 = qkv.shape
    d = D3 // (3 * heads)
    if not (qkv.is_contiguous() and cos.is_contiguous() and sin.is_contiguous() and cu_seqlens.is_contiguous()):
        raise RuntimeError("rope_attention_varlen needs contiguous operands")
    if cos.dtype != torch.float32 or sin.dtype != torch.float32 or cu_seqlens.dtype != torch.int32:
        raise RuntimeError("rope_attention_varlen: cos / sin must be fp32 and cu_seqlens int32")
    if cos.shape != (T, d) or sin.shape != (T, d) or cu_seqlens.device != qkv.device:
        raise RuntimeError(f"rope_attention_varlen: tables {tuple(cos.shape)} do not match [{T}, {d}]")
    if out is None:
        out = torch.empty(T, heads * d, dtype=qkv.dtype, device=qkv.device)
    S = cu_seqlens.numel() - 1
    # flops of the upper bound max_seqlen keys per query (the segment lengths stay on the device)
    L = max_seqlen if max_seqlen > 0 else T
    flops = 4 * heads * T * L * d
    nbytes = 4 * T * heads * d * 2 + 2 * T * d * 4
    waves = attention_waves(max_seqlen)
    with kernel_timer.region(f"rope_attention_varlen<bf16,{d},{waves}>", nbytes, flops, "mfma"):
        rc = _lib.vfm_rope_attention_varlen(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), cu_seqlens.data_ptr(),
                                            out.data_ptr(), T, heads, d, S, float(d) ** -0.5, int(max_seqlen),
                                            custom_ops.stream_ptr(qkv.device))
    custom_ops.check(rc, "vfm_rope_attention_varlen")
    return out


def rows_supported(h):
    return h.is_cuda and h.dtype in _DN and h.shape[-1] % 4 == 0 and h.shape[-1] <= 2048


def _weight(w):
    """fp32, contiguous, 16-B aligned norm weight, cached on the (frozen) parameter until its version moves."""
    from .decoder_hip import _cast_cached
    w = w.detach()
    w = w if w.dtype == torch.float32 else _cast_cached(w, torch.float32)
    w = w.contiguous()
    return w.clone() if w.data_ptr() % 16 else w


def rms_norm(h, delta, weight, eps, want_y=True):
    """(h_out, y): h_out = h + delta (h itself when delta is None), y = weight * rmsnorm(h_out) in h's dtype
    (None when want_y is False: the residual add alone). h, delta: [..., D] of one dtype (bf16 / fp32)."""
    _no_grad("rms_norm", h, delta)
    h = h.contiguous()
    D = h.shape[-1]
    rows = h.numel() // D
    h_out = None
    if delta is not None:
        if delta.shape != h.shape or delta.dtype != h.dtype:
            raise RuntimeError(f"rms_norm: delta {tuple(delta.shape)} {delta.dtype} != h {tuple(h.shape)} {h.dtype}")
        delta = delta.contiguous()
        h_out = torch.empty_like(h)
    y = torch.empty_like(h) if want_y else None
    w = _weight(weight) if want_y else None
    es = h.element_size()
    nbytes = rows * D * es * (1 + (2 if delta is not None else 0) + (1 if want_y else 0))
    with kernel_timer.region(f"rms_norm_rows<{_DN[h.dtype]}>", nbytes):
        rc = _lib.vfm_rms_norm_rows(h.data_ptr(), custom_ops.ptr(delta), custom_ops.ptr(h_out), custom_ops.ptr(w),
                                    custom_ops.ptr(y), custom_ops.dtype_code(h), rows, D, float(eps),
                                    custom_ops.stream_ptr(h.device))
    custom_ops.check(rc, "vfm_rms_norm_rows")
    return (h_out if h_out is not None else h), y


def swiglu(gu, inter):
    """gu: [..., 2 Ip] (gate | up) -> [..., Ip]: silu(gate) * up for columns < inter, zeros beyond."""
    _no_grad("swiglu", gu)
    gu = gu.contiguous()
    Ip = gu.shape[-1] // 2
    rows = gu.numel() // (2 * Ip)
    out = torch.empty(*gu.shape[:-1], Ip, dtype=gu.dtype, device=gu.device)
    with kernel_timer.region(f"swiglu_rows<{_DN[gu.dtype]}>", rows * Ip * 3 * gu.element_size()):
        rc = _lib.vfm_swiglu_rows(gu.data_ptr(), out.data_ptr(), custom_ops.dtype_code(gu), rows, int(inter), Ip,
                                  custom_ops.stream_ptr(gu.device))
    custom_ops.check(rc, "vfm_swiglu_rows")
    return out


def patch_gather(img, idx, patch, Kp, out_dtype):
    """img: fp32 [B, 3, H, W]; idx: int32 [T] raster patch ids -> [T, Kp] rows (out_dtype), K = 3 patch^2 real
    columns, the rest zero."""
    _no_grad("patch_gather", img)
    img = img.contiguous()
    B, C, H, W = img.shape
    if C != 3 or img.dtype != torch.float32 or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise RuntimeError("patch_gather: img must be fp32 [B, 3, H, W] and idx a contiguous int32 vector")
    T = idx.numel()
    out = torch.empty(T, Kp, dtype=out_dtype, device=img.device)
    K = 3 * patch * patch
    with kernel_timer.region(f"patch_gather<{_DN[out_dtype]}>", T * (K * 4 + Kp * out.element_size())):
        rc = _lib.vfm_patch_gather(img.data_ptr(), idx.data_ptr(), out.data_ptr(), custom_ops.dtype_code(out), B, H, W,
                                   patch, T, K, Kp, custom_ops.stream_ptr(img.device))
    custom_ops.check(rc, "vfm_patch_gather")
    return out
