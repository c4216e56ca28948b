"""fp64 restatements of the decoder kernel family (csrc/decoder.hip, dwconv_mfma.hip, rmsnorm.hip, torgb.hip,
posterior.hip) as explicit arithmetic: shifted products, sums and elementwise formulas, not calls to the op under
test. tests/test_decoder_refs.py pins every one of them against torch's own fp64 ops and autograd on the CPU;
tests/test_decoder_guard_gpu.py compares the kernels with them.

A plain module (like op_cases.py and guard_bands.py): no fixtures; tensors live where the inputs live. Every
function takes tensors of any float dtype, computes in float64 and returns float64 (split3 excepted: its point is
the bf16 bit patterns)."""
import math

import torch


def _d(t):
    return None if t is None else t.double()


# ---------------------------------------------------------------------------------------------- depthwise conv

def _zero_pad(x, pad):
    B, C, H, W = x.shape
    xp = x.new_zeros(B, C, H + 2 * pad, W + 2 * pad)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    return xp


def dwconv(x, w, bias=None, noise=None, res=None, pad=0, flip=False):
    """y[b, c] = sum_{ky, kx} w[c, ky, kx] xpad[b, c, ky:ky+Ho, kx:kx+Wo] (+ bias[c]) (+ noise [Ho, Wo]) (+ res);
    x [B, C, H, W], w [C, K, K] (flip: taps rotated by 180 degrees), zero padding `pad`."""
    x, w = _d(x), _d(w)
    B, C, H, W = x.shape
    K = w.shape[-1]
    if flip:
        w = w.flip(-1, -2)
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    xp = _zero_pad(x, pad)
    y = x.new_zeros(B, C, Ho, Wo)
    for ky in range(K):
        for kx in range(K):
            y.addcmul_(xp[:, :, ky:ky + Ho, kx:kx + Wo], w[:, ky, kx].reshape(1, C, 1, 1))
    if bias is not None:
        y += _d(bias).reshape(1, C, 1, 1)
    if noise is not None:
        y += _d(noise).reshape(1, 1, Ho, Wo)
    if res is not None:
        y += _d(res)
    return y


def dwconv_wgrad(x, dy, K, pad):
    """(dw [C, K, K], db [C]) of dwconv: dw[c, ky, kx] = sum_{b, y, x} dy[b, c] xpad[b, c, ky:ky+Ho, kx:kx+Wo],
    db[c] = sum dy[b, c]."""
    x, dy = _d(x), _d(dy)
    C = x.shape[1]
    Ho, Wo = dy.shape[-2:]
    xp = _zero_pad(x, pad)
    dw = x.new_zeros(C, K, K)
    for ky in range(K):
        for kx in range(K):
            dw[:, ky, kx] = (dy * xp[:, :, ky:ky + Ho, kx:kx + Wo]).sum((0, 2, 3))
    return dw, dy.sum((0, 2, 3))


# ---------------------------------------------------------------------------------------------- GroupNorm

def group_norm_fwd(x, G, w=None, b=None, s=None, eps=1e-5):
    """(y, mean [B G], rstd [B G]): y = ((x - mean) rstd w[c] + b[c]) s[b, c], biased variance over each group."""
    x = _d(x)
    B, C = x.shape[:2]
    xg = x.reshape(B, G, -1)
    n = xg.shape[-1]
    mean = xg.sum(-1) / n
    var = ((xg - mean[:, :, None]) ** 2).sum(-1) / n
    rstd = 1.0 / torch.sqrt(var + eps)
    y = ((xg - mean[:, :, None]) * rstd[:, :, None]).reshape(B, C, -1)
    if w is not None:
        y = y * _d(w)[None, :, None]
    if b is not None:
        y = y + _d(b)[None, :, None]
    if s is not None:
        y = y * _d(s)[:, :, None]
    return y.reshape(x.shape), mean.reshape(-1), rstd.reshape(-1)


def group_norm_bwd(x, dy, G, w=None, b=None, s=None, eps=1e-5):
    """(dx, dw_part [B, C], db_part [B, C], ds [B, C]): with xhat = (x - mean) rstd, A = sum_p dy xhat, S = sum_p dy,
    k = w s: dw_part = s A, db_part = s S, ds = w A + b S, and per group of n elements
    dx = rstd (k dy - sum(k S) / n - xhat sum(k A) / n)."""
    x, dy = _d(x), _d(dy)
    B, C = x.shape[:2]
    xhat, _, rstd = group_norm_fwd(x, G, eps=eps)
    xhat, dy3 = xhat.reshape(B, C, -1), dy.reshape(B, C, -1)
    n = (C // G) * xhat.shape[-1]
    one = x.new_ones(())
    wv = one.expand(C) if w is None else _d(w)
    bv = 0 * one.expand(C) if b is None else _d(b)
    sv = one.expand(B, C) if s is None else _d(s)
    A, S = (dy3 * xhat).sum(-1), dy3.sum(-1)
    k = wv[None] * sv
    m1 = (k * S).reshape(B, G, -1).sum(-1) / n
    m2 = (k * A).reshape(B, G, -1).sum(-1) / n
    rep = C // G
    m1c, m2c, rc = (t.reshape(B, G).repeat_interleave(rep, 1)[:, :, None] for t in (m1, m2, rstd))
    dx = rc * (k[:, :, None] * dy3 - m1c - xhat * m2c)
    return dx.reshape(x.shape), sv * A, sv * S, wv[None] * A + bv[None] * S


# ---------------------------------------------------------------------------------------------- row ops

def _z(h, scale, bias):
    z = _d(h)
    if scale is not None:
        z = z * _d(scale)[:, :, None]
    if bias is not None:
        z = z + _d(bias)[None, :, None]
    return z


def gelu_fwd(h, scale=None, bias=None):
    """g = z Phi(z), z = h scale[b, o] + bias[o] on h [B, O, P]; Phi the standard normal CDF (erf form)."""
    z = _z(h, scale, bias)
    return z * 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_bwd(h, dg, scale=None, bias=None):
    """(dh, d_scale_rows [B, O], d_bias_rows [B, O]): dz = dg (Phi(z) + z phi(z)), dh = dz scale,
    d_scale_rows = sum_p dz h, d_bias_rows = sum_p dz."""
    z = _z(h, scale, bias)
    cdf = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    dz = _d(dg) * (cdf + z * pdf)
    dh = dz if scale is None else dz * _d(scale)[:, :, None]
    return dh, (dz * _d(h)).sum(-1), dz.sum(-1)


def lsr_fwd(y, bias, gamma, x_in):
    """out = x_in + gamma[c] (y + bias[c]) on [B, C, P]."""
    t = _d(y)
    if bias is not None:
        t = t + _d(bias)[None, :, None]
    if gamma is not None:
        t = t * _d(gamma)[None, :, None]
    return _d(x_in) + t


def lsr_bwd(y, bias, gamma, dout):
    """(dy, d_gamma_rows [B, C], d_sum_rows [B, C]): dy = gamma dout, sum_p (y + bias) dout, sum_p dout."""
    dout, t = _d(dout), _d(y)
    if bias is not None:
        t = t + _d(bias)[None, :, None]
    dy = dout if gamma is None else dout * _d(gamma)[None, :, None]
    return dy, (t * dout).sum(-1), dout.sum(-1)


# ---------------------------------------------------------------------------------------------- shuffle + blur

def _blur_setup(taps, dev):
    k = torch.tensor([float(t) for t in taps], dtype=torch.float64, device=dev)
    k = k / k.sum()
    K = k.numel()
    p0 = (K - 1) // 2

    def idx(size):        # replicate pad: padded position -> source position
        return torch.arange(-p0, size + K - 1 - p0, device=dev).clamp(0, size - 1)

    return k, K, idx


def shuffle_blur_fwd(x, taps, r):
    """PixelShuffle(r) (ps[b, c, h r + i, w r + j] = x[b, c r^2 + i r + j, h, w]), replicate pad ((K-1)/2 before,
    K/2 after), then y = sum_{ky, kx} k[ky] k[kx] pad[ky:ky+Hr, kx:kx+Wr] with k = taps / sum(taps)."""
    x = _d(x)
    B, Cr, H, W = x.shape
    C = Cr // (r * r)
    ps = x.reshape(B, C, r, r, H, W).permute(0, 1, 4, 2, 5, 3).reshape(B, C, H * r, W * r)
    k, K, idx = _blur_setup(taps, x.device)
    Hr, Wr = H * r, W * r
    xp = ps[:, :, idx(Hr)][:, :, :, idx(Wr)]
    y = x.new_zeros(B, C, Hr, Wr)
    for ky in range(K):
        for kx in range(K):
            y += k[ky] * k[kx] * xp[:, :, ky:ky + Hr, kx:kx + Wr]
    return y


def shuffle_blur_bwd(dout, taps, r):
    """The exact adjoint: dout [B, C, H r, W r] -> dx [B, C r^2, H, W]: every tap's product scattered to the padded
    plane, the pad's copies summed back onto their source rows / columns, the shuffle undone."""
    dout = _d(dout)
    B, C, Hr, Wr = dout.shape
    H, W = Hr // r, Wr // r
    k, K, idx = _blur_setup(taps, dout.device)
    dxp = dout.new_zeros(B, C, Hr + K - 1, Wr + K - 1)
    for ky in range(K):
        for kx in range(K):
            dxp[:, :, ky:ky + Hr, kx:kx + Wr] += k[ky] * k[kx] * dout
    rows = dout.new_zeros(B, C, Hr, Wr + K - 1).index_add_(2, idx(Hr), dxp)
    dps = dout.new_zeros(B, C, Hr, Wr).index_add_(3, idx(Wr), rows)
    return dps.reshape(B, C, H, r, W, r).permute(0, 1, 3, 5, 2, 4).reshape(B, C * r * r, H, W)


# ---------------------------------------------------------------------------------------------- channel RMS norm

NORM_EPS = 1e-12


def rms_fwd(x, gamma, scale):
    """(y, rinv [B, P]): n = max(sqrt(sum_c x^2), 1e-12), y = x / n scale gamma[c], rinv = 1 / n; x [B, C, P]."""
    x = _d(x)
    rinv = 1.0 / torch.sqrt((x * x).sum(1)).clamp_min(NORM_EPS)
    return x * rinv[:, None, :] * (scale * _d(gamma))[None, :, None], rinv


def rms_bwd(x, gamma, dy, scale):
    """(dx, dgamma [C]): k = scale gamma; dx = k dy / n - x (sum_c k dy x) / n^3 where the norm is not clamped and
    k dy / n where it is; dgamma = scale sum_{b, p} dy x / n."""
    x, dy = _d(x), _d(dy)
    k = (scale * _d(gamma))[None, :, None]
    norm = torch.sqrt((x * x).sum(1))
    rinv = 1.0 / norm.clamp_min(NORM_EPS)
    dot = (k * dy * x).sum(1)
    corr = torch.where(norm > NORM_EPS, dot * rinv ** 3, torch.zeros_like(dot))
    dx = k * dy * rinv[:, None, :] - x * corr[:, None, :]
    return dx, scale * (dy * x * rinv[:, None, :]).sum((0, 2))


# ---------------------------------------------------------------------------------------------- ToRGB

def torgb_fwd(x, wm, bias, round_bf16=None):
    """y[b, o, p] = r(sum_c wm[b, o, c] x[b, c, p]) + bias[o]; r rounds the sum to bf16 when x is bf16 (default:
    by x's dtype), the bf16 product of the reference before its fp32 bias."""
    if round_bf16 is None:
        round_bf16 = x.dtype == torch.bfloat16
    x, wm = _d(x), _d(wm)
    acc = (wm[:, :, :, None] * x[:, None, :, :]).sum(2)
    if round_bf16:
        acc = acc.float().bfloat16().double()
    return acc + _d(bias)[None, :, None]


def torgb_bwd(x, dy, wm):
    """(dx [B, C, P] = sum_o wm dy, T [B, O, C] = sum_p x dy)."""
    x, dy, wm = _d(x), _d(dy), _d(wm)
    dx = (wm[:, :, :, None] * dy[:, :, None, :]).sum(1)
    O = wm.shape[1]
    T = torch.stack([(x * dy[:, o:o + 1, :]).sum(-1) for o in range(O)], 1)
    return dx, T


# ---------------------------------------------------------------------------------------------- posterior

LV_MIN, LV_MAX = -30.0, 20.0


def posterior_fwd(params, eps):
    """(z, kl [B]): params [B, 2C, P] = mean | logvar, lv = clamp(logvar, -30, 20), z = mean + exp(lv / 2) eps,
    kl = 0.5 sum_{c, p} (mean^2 + exp(lv) - 1 - lv)."""
    p = _d(params)
    C = p.shape[1] // 2
    m, raw = p[:, :C], p[:, C:]
    lv = torch.minimum(torch.maximum(raw, raw.new_tensor(LV_MIN)), raw.new_tensor(LV_MAX))
    z = m + torch.exp(0.5 * lv) * _d(eps)
    return z, 0.5 * (m * m + torch.exp(lv) - 1.0 - lv).sum((1, 2))


def posterior_bwd(params, eps, dz=None, dkl=None):
    """dparams [B, 2C, P]: dmean = dz + dkl[b] mean; dlogvar = (dz eps exp(lv / 2) + dkl[b] (exp(lv) - 1)) / 2 where
    -30 <= logvar <= 20 and 0 beyond the clamps. dz or dkl None: that term is zero."""
    p = _d(params)
    C = p.shape[1] // 2
    m, raw = p[:, :C], p[:, C:]
    lv = torch.minimum(torch.maximum(raw, raw.new_tensor(LV_MIN)), raw.new_tensor(LV_MAX))
    g = torch.zeros_like(m) if dz is None else _d(dz)
    k = (torch.zeros_like(m[:, 0, 0]) if dkl is None else _d(dkl))[:, None, None]
    dlv = 0.5 * (g * _d(eps) * torch.exp(0.5 * lv) + k * (torch.exp(lv) - 1.0))
    inside = (raw >= LV_MIN) & (raw <= LV_MAX)
    return torch.cat([g + k * m, torch.where(inside, dlv, torch.zeros_like(dlv))], 1)


# ---------------------------------------------------------------------------------------------- bf16 pieces

def split3(t):
    """The planar bf16 pieces [3, numel] of an fp32 tensor: hi = bf16(t), mid = bf16(t - hi), lo = bf16(t - hi - mid)
    (round to nearest even; both remainders are exact in fp32), so that hi + mid + lo == t exactly."""
    assert t.dtype == torch.float32
    t = t.reshape(-1)
    hi = t.bfloat16()
    r1 = t - hi.float()
    mid = r1.bfloat16()
    lo = (r1 - mid.float()).bfloat16()
    return torch.stack([hi, mid, lo])
