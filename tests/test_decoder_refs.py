"""tests/decoder_refs.py against torch's own fp64 CPU ops and autograd, to 1e-12 relative, on tiny shapes: pins the
references tests/test_decoder_guard_gpu.py compares the decoder kernels with, without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import decoder_refs as R

TOL = 1e-12


def _close(a, b, what=""):
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert a.shape == b.shape and err < TOL, (what, err)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("K,pad", [(3, 1), (5, 2), (7, 3), (3, 0), (7, 1)])
@pytest.mark.parametrize("flip", [False, True])
def test_dwconv(K, pad, flip):
    g = torch.Generator().manual_seed(K + pad)
    B, C, H, W = 2, 3, 9, 11
    x, w, b = _rand(g, B, C, H, W).requires_grad_(), _rand(g, C, K, K).requires_grad_(), _rand(g, C).requires_grad_()
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    noise, res, dy = _rand(g, Ho, Wo), _rand(g, B, C, Ho, Wo), _rand(g, B, C, Ho, Wo)
    wt = w.flip(-1, -2) if flip else w
    y = F.conv2d(x, wt[:, None], b, padding=pad, groups=C) + noise + res
    _close(R.dwconv(x.detach(), w.detach(), b.detach(), noise, res, pad, flip), y.detach(), "y")
    _close(R.dwconv(x.detach(), w.detach(), pad=pad, flip=flip),
           F.conv2d(x, wt[:, None], None, padding=pad, groups=C).detach(), "plain")
    y.backward(dy)
    if not flip:
        dw, db = R.dwconv_wgrad(x.detach(), dy, K, pad)
        _close(dw, w.grad, "dw")
        _close(db, b.grad, "db")
    # the data gradient is the same conv of dy with the rotated taps and pad' = K - 1 - pad
    _close(R.dwconv(dy, w.detach(), pad=K - 1 - pad, flip=not flip), x.grad, "dx")


@pytest.mark.parametrize("shape,G", [((2, 8, 4, 4), 1), ((2, 12, 5, 7), 3), ((2, 8, 1, 1), 2), ((1, 6, 3, 2), 6)])
@pytest.mark.parametrize("affine,style", [(True, True), (True, False), (False, True), (False, False)])
def test_group_norm(shape, G, affine, style):
    g = torch.Generator().manual_seed(sum(shape) + G)
    B, C = shape[:2]
    x = (_rand(g, *shape) * 3 + 1.5).requires_grad_()
    # per-sample copies of the affine parameters: their gradients are the per-sample parts
    w = (1 + 0.1 * _rand(g, C)) if affine else None
    b = (0.1 * _rand(g, C)) if affine else None
    s = (1 + 0.3 * _rand(g, B, C)).requires_grad_() if style else None
    wb = w.expand(B, C).clone().requires_grad_() if affine else None
    bb = b.expand(B, C).clone().requires_grad_() if affine else None
    dy = _rand(g, *shape)
    y = F.group_norm(x, G, None, None, 1e-5)
    if affine:
        y = y * wb[:, :, None, None] + bb[:, :, None, None]
    if style:
        y = y * s[:, :, None, None]
    y.backward(dy)
    yr, mean, rstd = R.group_norm_fwd(x.detach(), G, w, b, None if s is None else s.detach())
    _close(yr, y.detach(), "y")
    if affine:
        _close(R.group_norm_fwd(x.detach(), G, w, b)[0], F.group_norm(x.detach(), G, w, b, 1e-5), "affine")
    xg = x.detach().reshape(B * G, -1)
    _close(mean, xg.mean(1), "mean")
    _close(rstd, (xg.var(1, unbiased=False) + 1e-5).rsqrt(), "rstd")
    dx, dwp, dbp, ds = R.group_norm_bwd(x.detach(), dy, G, w, b, None if s is None else s.detach())
    if xg.shape[1] > 1:
        _close(dx, x.grad, "dx")
    else:       # one element per group: dx is zero up to cancellation
        assert float(dx.abs().max()) < 1e-9 and float(x.grad.abs().max()) < 1e-9
    if affine:
        _close(dwp, wb.grad, "dw_part")
        _close(dbp, bb.grad, "db_part")
    if style:
        _close(ds, s.grad, "ds")


@pytest.mark.parametrize("with_scale,with_bias", [(True, True), (False, True), (True, False), (False, False)])
def test_gelu(with_scale, with_bias):
    g = torch.Generator().manual_seed(5)
    B, O, P = 2, 3, 8
    h = (_rand(g, B, O, P) * 2).requires_grad_()
    s = (torch.rand(B, O, generator=g, dtype=torch.float64) + 0.5).requires_grad_()
    b = 0.3 * _rand(g, O)
    bb = b.expand(B, O).clone().requires_grad_()
    dg = _rand(g, B, O, P)
    z = h * s[:, :, None] if with_scale else h * 1.0
    z = z + bb[:, :, None] if with_bias else z
    out = F.gelu(z)
    out.backward(dg)
    sa, ba = (s.detach() if with_scale else None), (b if with_bias else None)
    _close(R.gelu_fwd(h.detach(), sa, ba), out.detach(), "g")
    dh, r0, r1 = R.gelu_bwd(h.detach(), dg, sa, ba)
    _close(dh, h.grad, "dh")
    if with_scale:
        _close(r0, s.grad, "d_scale_rows")
    if with_bias:
        _close(r1, bb.grad, "d_bias_rows")


def test_layer_scale_residual():
    g = torch.Generator().manual_seed(6)
    B, C, P = 2, 3, 8
    y, x = _rand(g, B, C, P).requires_grad_(), _rand(g, B, C, P)
    b, gm = 0.1 * _rand(g, C), 0.5 + 0.2 * _rand(g, C)
    bb = b.expand(B, C).clone().requires_grad_()
    gb = gm.expand(B, C).clone().requires_grad_()
    dout = _rand(g, B, C, P)
    out = x + gb[:, :, None] * (y + bb[:, :, None])
    out.backward(dout)
    _close(R.lsr_fwd(y.detach(), b, gm, x), out.detach(), "out")
    _close(R.lsr_fwd(y.detach(), None, None, x), (x + y).detach(), "plain")
    dy, r0, r1 = R.lsr_bwd(y.detach(), b, gm, dout)
    _close(dy, y.grad, "dy")
    _close(r0, gb.grad, "d_gamma_rows")
    _close(r1 * gm[None], bb.grad, "d_sum_rows")


@pytest.mark.parametrize("taps", [[1, 1], [1, 2, 1], [1, 3, 3, 1], [1, 4, 6, 4, 1], [1, 7, 21, 35, 35, 21, 7, 1]])
@pytest.mark.parametrize("shape,r", [((1, 4, 1, 1), 2), ((2, 12, 5, 7), 2), ((2, 3, 4, 9), 1), ((1, 4, 3, 8), 2)])
def test_shuffle_blur(shape, r, taps):
    g = torch.Generator().manual_seed(7)
    x = _rand(g, *shape).requires_grad_()
    k = torch.tensor(taps, dtype=torch.float64)
    k2 = torch.outer(k, k) / k.sum() ** 2
    K = len(taps)
    p0, p1 = (K - 1) // 2, K // 2
    ps = F.pixel_shuffle(x, r)
    C = ps.shape[1]
    y = F.conv2d(F.pad(ps, (p0, p1, p0, p1), mode="replicate"), k2[None, None].repeat(C, 1, 1, 1), groups=C)
    dout = _rand(g, *y.shape)
    y.backward(dout)
    _close(R.shuffle_blur_fwd(x.detach(), taps, r), y.detach(), "y")
    _close(R.shuffle_blur_bwd(dout, taps, r), x.grad, "dx")


def test_channel_rms_norm():
    g = torch.Generator().manual_seed(8)
    B, C, P, scale = 2, 5, 7, 5 ** 0.5
    x0 = _rand(g, B, C, P)
    x0[1, :, 3] = 0.0                                   # a clamped column
    x = x0.clone().requires_grad_()
    gamma = (1 + 0.2 * _rand(g, C)).requires_grad_()
    dy = _rand(g, B, C, P)
    y = F.normalize(x, dim=1, eps=1e-12) * scale * gamma[None, :, None]
    y.backward(dy)
    yr, rinv = R.rms_fwd(x0, gamma.detach(), scale)
    _close(yr, y.detach(), "y")
    assert float(yr[1, :, 3].abs().max()) == 0.0 and float(rinv[1, 3]) == 1e12
    _close(rinv, 1.0 / x0.norm(dim=1).clamp_min(1e-12), "rinv")
    dx, dgm = R.rms_bwd(x0, gamma.detach(), dy, scale)
    _close(dx, x.grad, "dx")
    _close(dx[1, :, 3], (scale * gamma.detach() * dy[1, :, 3]) * 1e12, "clamped column")
    _close(dgm, gamma.grad, "dgamma")


@pytest.mark.parametrize("O", [1, 3, 4])
def test_torgb(O):
    g = torch.Generator().manual_seed(9)
    B, C, P = 2, 16, 8
    x = _rand(g, B, C, P).requires_grad_()
    wm = (0.1 * _rand(g, B, O, C)).requires_grad_()
    bias, dy = _rand(g, O), _rand(g, B, O, P)
    y = torch.matmul(wm, x) + bias[None, :, None]
    y.backward(dy)
    _close(R.torgb_fwd(x.detach(), wm.detach(), bias), y.detach(), "y")
    dx, T = R.torgb_bwd(x.detach(), dy, wm.detach())
    _close(dx, x.grad, "dx")
    _close(T, wm.grad, "T")
    # bf16 planes: the product rounded to bf16 before the fp32 bias
    xb = x.detach().bfloat16()
    want = torch.matmul(wm.detach(), xb.double()).float().bfloat16().double() + bias[None, :, None]
    _close(R.torgb_fwd(xb, wm.detach(), bias), want, "bf16 product")


def test_posterior():
    g = torch.Generator().manual_seed(10)
    B, C, P = 3, 4, 6
    p0 = _rand(g, B, 2 * C, P)
    p0[:, C:, 0] = 25.0
    p0[:, C:, 1] = -35.0
    p0[0, C, 2], p0[0, C, 3] = 20.0, -30.0             # on the clamps: gradient flows (torch.clamp's convention)
    params = p0.clone().requires_grad_()
    eps, dz, dkl = _rand(g, B, C, P), _rand(g, B, C, P), _rand(g, B)
    mean, logvar = params[:, :C], torch.clamp(params[:, C:], -30.0, 20.0)
    z = mean + torch.exp(0.5 * logvar) * eps
    kl = 0.5 * torch.sum(mean ** 2 + torch.exp(logvar) - 1.0 - logvar, dim=[1, 2])
    zr, klr = R.posterior_fwd(p0, eps)
    _close(zr, z.detach(), "z")
    _close(klr, kl.detach(), "kl")
    for use_z, use_k in ((True, True), (True, False), (False, True)):
        params.grad = None
        ((z * dz).sum() * float(use_z) + (kl * dkl).sum() * float(use_k)).backward(retain_graph=True)
        got = R.posterior_bwd(p0, eps, dz if use_z else None, dkl if use_k else None)
        _close(got, params.grad, f"dparams z={use_z} kl={use_k}")
        assert float(got[:, C:, :2].abs().max()) == 0.0


def test_split3_is_exact_and_rounds_to_nearest():
    g = torch.Generator().manual_seed(11)
    t = torch.randn(4, 8, 16, generator=g) * torch.logspace(-6, 6, 16)
    p = R.split3(t)
    assert p.shape == (3, t.numel()) and p.dtype == torch.bfloat16
    assert torch.equal(p[0], t.reshape(-1).bfloat16())
    assert torch.equal(p.double().sum(0), t.reshape(-1).double())       # hi + mid + lo == t, exactly
    assert float((p[1].double().abs() / p[0].double().abs()).max()) <= 2.0 ** -8
