"""Attention over a short key list under a key-padding mask (csrc/xattn.hip).

  keymask_attention_packed  the SigLIP2 text tower's self-attention (HF SiglipTextModel with attention_mask
                            under bf16 autocast): bf16, head dim 64, N <= 128, forward only.
  cross_attention           the decoder's text cross-attention with its learned null key / value (reference
                            networks/utils/gigagan_utils.py:94-146 CrossAttention.forward) as ONE autograd
                            Function, laid out like gigaattn_hip._NullKVSelfAttention so that no activation is
                            copied between the products:

  forward   q[b] = (W_q x[b])^T          token-major [P, h d], written by the projection GEMM itself
            kv[b] = ctx[b] W_kv^T        [L, 2 h d], read in place ([L, 2, h, d]: chunk(2) = all of k, then v)
            o = attention(q, [null_k; k], [null_v; v], mask)   the null row and the mask are read by the kernel
            y[b] = W_out o[b]^T          [C, P], channel-first
  backward  dW_out = sum_b dy[b] o[b];  do[b] = (W_out^T dy[b])^T;  attention backward -> dq, dkv (packed as
            kv), dnull;  dW_q = sum_b dq[b]^T x[b]^T;  dx[b] = W_q^T dq[b]^T;  dW_kv = sum_b dkv[b]^T ctx[b];
            dctx[b] = dkv[b] W_kv

The reference module prepends a FALSE column to its boolean mask, so whenever it is given a mask the null key
is masked out as well (it takes part only in the unmasked call). `cross_attention` computes exactly that
(mask_null = key_mask is not None); the kernels' own contract (mask_null = 0: the null key is never masked) is
what `cross_attention_core` exposes.

VFM_XATTN=torch keeps the torch formulation (two torch.cat, an expanded boolean mask, F.scaled_dot_product_
attention) on ROCm tensors (A/B, tools_dev/xattnbench.py); the default is hip.
"""
import os

import torch

from .. import custom_ops
from . import kernel_timer
from .attn_hip import _lib, _s4, _strides
from .gigaattn_hip import _mm

OWN = os.environ.get("VFM_XATTN", "hip")
if OWN not in ("hip", "torch"):
    raise ValueError(f"VFM_XATTN must be hip or torch, not {OWN!r}")
MAX_KEYS = 128


def _mask_ptr(key_mask, B, L):
    """(tensor kept alive, pointer) of a [B, L] uint8 mask (torch.bool storage is one 0 / 1 byte an element)."""
    if key_mask is None:
        return None, None
    if key_mask.shape != (B, L):
        raise RuntimeError(f"key mask {tuple(key_mask.shape)} does not match [B, L] = {(B, L)}")
    m = key_mask if key_mask.dtype in (torch.bool, torch.uint8) else key_mask != 0
    m = m.contiguous()
    return m, m.data_ptr()


# ------------------------------------------------------------------------------------------------ text tower

def keymask_supported(x, head_dim, n):
    return x.is_cuda and x.dtype == torch.bfloat16 and head_dim == 64 and n <= MAX_KEYS


def keymask_attention_packed(qkv, heads, key_mask, out=None):
    """qkv: bf16 [B, N, 3*D] (q | k | v, heads contiguous inside each), key_mask [B, N] (non-zero = attend) or
    None -> [B, N, D]. Every sample needs one valid key."""
    if torch.is_grad_enabled() and qkv.requires_grad:
        raise RuntimeError("xattn_hip.keymask_attention_packed is forward-only (frozen text tower under no_grad)")
    B, N, D3 = qkv.shape
    D = D3 // 3
    d = D // heads
    v5 = qkv.view(B, N, 3, heads, d)
    q, k, v = v5[:, :, 0], v5[:, :, 1], v5[:, :, 2]
    if out is None:
        out = torch.empty(B, N, heads, d, dtype=qkv.dtype, device=qkv.device)
    keep, mp = _mask_ptr(key_mask, B, N)
    with kernel_timer.region(f"attention_keymask_fwd<bf16,{d}>", 4 * B * N * D * qkv.element_size() + B * N,
                             4 * B * heads * N * N * d, "mfma"):
        rc = _lib.vfm_attention_keymask_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), mp, out.data_ptr(), B, heads, N,
                                            d, _strides(q), _strides(k), _strides(v), _strides(out), float(d) ** -0.5,
                                            custom_ops.stream_ptr(qkv.device))
    custom_ops.check(rc, "vfm_attention_keymask_fwd")
    return out.view(B, N, D)


# ------------------------------------------------------------------------------------------------ decoder

def _workspace(B, H, Nq, L, d, device):
    n = _lib.vfm_cross_attention_f32_workspace_floats(B, H, Nq, L, d)
    if n < 0:
        raise custom_ops.NativeError(f"vfm_cross_attention_f32_workspace_floats failed with code {n}")
    return torch.empty(n, dtype=torch.float32, device=device)


def _core_fwd(q, kv, null_kv, key_mask, mask_null, o=None):
    B, Nq, H, d = q.shape
    L = kv.shape[1]
    if o is None:
        o = torch.empty(B, Nq, H, d, dtype=torch.float32, device=q.device)
    lse = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device)
    keep, mp = _mask_ptr(key_mask, B, L)
    prec, _, tag = custom_ops.f32_precision()
    with kernel_timer.region(f"cross_attention_fwd<{tag},{d}>", 4 * (2 * B * Nq * H * d + 2 * (B * L + 1) * H * d),
                             4 * B * H * Nq * (L + 1) * d, "mfma"):
        rc = _lib.vfm_cross_attention_f32_fwd(q.data_ptr(), kv.data_ptr(), null_kv.data_ptr(), mp, o.data_ptr(),
                                              lse.data_ptr(), B, H, Nq, L, d, _s4(q), _s4(o), float(d) ** -0.5,
                                              int(mask_null), prec, custom_ops.stream_ptr(q.device))
    custom_ops.check(rc, "vfm_cross_attention_f32_fwd")
    return o, lse


def _core_bwd(q, kv, null_kv, key_mask, mask_null, o, do, lse, dq=None, dkv=None, dnull=None):
    B, Nq, H, d = q.shape
    L = kv.shape[1]
    if dq is None:
        dq = torch.empty(B, Nq, H, d, dtype=torch.float32, device=q.device)
    if dkv is None:
        dkv = torch.empty(B, L, 2, H, d, dtype=torch.float32, device=q.device)
    if dnull is None:
        dnull = torch.empty(2, H, d, dtype=torch.float32, device=q.device)
    ws = _workspace(B, H, Nq, L, d, q.device)
    keep, mp = _mask_ptr(key_mask, B, L)
    prec, _, tag = custom_ops.f32_precision()
    # S and dP in both passes, dV, dK, dQ; q, o, do, dq and kv / dkv once each plus the partials
    with kernel_timer.region(f"cross_attention_bwd<{tag},{d}>",
                             4 * (4 * B * Nq * H * d + 4 * B * (L + 1) * H * d) + 8 * ws.numel(),
                             10 * B * H * Nq * (L + 1) * d, "mfma"):
        rc = _lib.vfm_cross_attention_f32_bwd(q.data_ptr(), kv.data_ptr(), null_kv.data_ptr(), mp, o.data_ptr(),
                                              do.data_ptr(), lse.data_ptr(), ws.data_ptr(), dq.data_ptr(),
                                              dkv.data_ptr(), dnull.data_ptr(), B, H, Nq, L, d, _s4(q), _s4(o),
                                              _s4(do), _s4(dq), float(d) ** -0.5, int(mask_null), prec,
                                              custom_ops.stream_ptr(q.device))
    custom_ops.check(rc, "vfm_cross_attention_f32_bwd")
    return dq, dkv, dnull


class _CrossAttentionCore(custom_ops.FastFunction):
    """The attention alone: q [B, Nq, H, d], kv [B, L, 2, H, d] contiguous, null_kv [2, H, d] -> o [B, Nq, H, d]."""

    @staticmethod
    def forward(ctx, q, kv, null_kv, key_mask, mask_null):
        if _s4(q) is None:
            q = q.contiguous()
        kv, null_kv = kv.contiguous(), null_kv.contiguous()
        o, lse = _core_fwd(q, kv, null_kv, key_mask, mask_null)
        ctx.save_for_backward(q, kv, null_kv, o, lse)
        ctx.key_mask, ctx.mask_null = key_mask, mask_null
        return o

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, do):
        q, kv, null_kv, o, lse = ctx.saved_tensors
        if _s4(do) is None:
            do = do.contiguous()
        dq, dkv, dnull = _core_bwd(q, kv, null_kv, ctx.key_mask, ctx.mask_null, o, do, lse)
        return dq, dkv, dnull, None, None


def cross_attention_core(q, kv, null_kv, key_mask=None, mask_null=False):
    """softmax over [null ; text keys] under key_mask [B, L] (non-zero = attend; None: no mask), fp32, forward and
    backward. mask_null False: the null key is never masked."""
    return _CrossAttentionCore.apply(q, kv, null_kv, key_mask, mask_null)


class _CrossAttention(custom_ops.FastFunction):
    @staticmethod
    def forward(ctx, x3, wq, wkv, context, null_kv, wout, key_mask, heads):
        B, C, P = x3.shape
        hd = wq.shape[0]
        d = hd // heads
        L = context.shape[1]
        q = _mm(x3.transpose(1, 2), wq.detach().t(), cache_b=True)                   # [B, P, hd] token-major
        kv = _mm(context.detach(), wkv.detach().t(), cache_b=True)                   # [B, L, 2 hd]
        nkv = null_kv.detach().to(torch.float32).contiguous()
        q4, kv5 = q.view(B, P, heads, d), kv.view(B, L, 2, heads, d)
        o, lse = _core_fwd(q4, kv5, nkv, key_mask, key_mask is not None)
        y = _mm(wout.detach(), o.view(B, P, hd).transpose(1, 2), cache_a=True)       # [B, C, P]
        ctx.save_for_backward(x3, wq, wkv, context, nkv, wout, q, kv, o, lse)
        ctx.heads, ctx.key_mask = heads, key_mask
        ctx.dtypes = (wq.dtype, wkv.dtype, null_kv.dtype, wout.dtype)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x3, wq, wkv, context, nkv, wout, q, kv, o, lse = ctx.saved_tensors
        heads, key_mask = ctx.heads, ctx.key_mask
        B, C, P = x3.shape
        hd = wq.shape[0]
        d = hd // heads
        L = context.shape[1]
        need = ctx.needs_input_grad
        dy = dy.contiguous()
        dwout = _mm(dy, o.view(B, P, hd), out_dtype=torch.float32, reduce_batch=True) if need[5] else None
        do = _mm(dy.transpose(1, 2), wout.detach(), cache_b=True)                    # [B, P, hd] token-major
        dq4, dkv5, dnull = _core_bwd(q.view(B, P, heads, d), kv.view(B, L, 2, heads, d), nkv, key_mask,
                                     key_mask is not None, o, do.view(B, P, heads, d), lse)
        dq, dkv = dq4.view(B, P, hd), dkv5.view(B, L, 2 * hd)
        qdt, kdt, ndt, odt = ctx.dtypes
        dx = _mm(wq.detach().t(), dq.transpose(1, 2), cache_a=True) if need[0] else None
        dwq = _mm(dq.transpose(1, 2), x3.transpose(1, 2), out_dtype=torch.float32,
                  reduce_batch=True).to(qdt) if need[1] else None
        dwkv = _mm(dkv.transpose(1, 2), context.detach(), out_dtype=torch.float32,
                   reduce_batch=True).to(kdt) if need[2] else None
        dctx = _mm(dkv, wkv.detach(), cache_b=True) if need[3] else None
        return (dx, dwq, dwkv, dctx, dnull.to(ndt) if need[4] else None, None if dwout is None else dwout.to(odt),
                None, None)


def supported(x3, context, heads, dim_head):
    """ROCm fp32 operands in the kernels' range (d in {32, 64}, L + 1 <= 128, 16-B rows) and VFM_XATTN != torch."""
    return (OWN == "hip" and x3.is_cuda and x3.dtype == torch.float32 and context.dtype == torch.float32
            and dim_head in (32, 64) and context.shape[1] + 1 <= MAX_KEYS and context.shape[1] >= 1
            and x3.shape[1] % 4 == 0 and x3.shape[2] % 4 == 0 and context.shape[2] % 4 == 0)


def cross_attention(x3, wq, wkv, context, null_kv, wout, key_mask, heads):
    """y [B, C, P] = W_out attention(W_q x3, [null_k; k], [null_v; v]) with (k, v) = chunk(context W_kv^T):
    x3 [B, C, P] fp32 (normalised feature map), wq [h d, C], wkv [2 h d, Dc], context [B, L, Dc] (normalised text
    tokens), null_kv [2, h, d], wout [C, h d], key_mask bool [B, L] or None. With a mask the null key is masked
    too, as in the reference module."""
    return _CrossAttention.apply(x3, wq, wkv, context, null_kv, wout, key_mask, heads)
