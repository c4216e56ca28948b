"""Fused Gaussian SSIM loss kernels (csrc/ssim.hip) behind training.loss.SSIM on the GPU.

Reference: SSIM(data_range=2.0) on the CPU in fp64 with .clamp(-1, 1) applied beforehand (the reference's
call, training/loss.py:257-260). Noise-case bounds are the project's for its fp32 fused loss kernels
(test_posterior_sample_kl): |value - ref| <= 1e-6 and ||grad - ref|| / ||ref|| <= 1e-5."""
import functools
import os
import types

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from conftest import ROOT  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
VALUE_TOL, GRAD_TOL = 1e-6, 1e-5


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _tiles():
    from torch_utils.ops import ssim_hip
    return ssim_hip.TILE_H, ssim_hip.TILE_W


def _noise_shapes():
    th, tw = _tiles()
    return {"one_pixel": (2, 3, 11, 11), "partial_tile": (1, 3, 12, 37), "ragged": (2, 1, 45, 70),
            "tiles_plus_rest": (1, 2, 2 * th + 13, 3 * tw + 11), "workload_plane": (1, 3, 256, 256)}


NOISE_CASES = ["one_pixel", "partial_tile", "ragged", "tiles_plus_rest", "workload_plane"]


@functools.lru_cache(maxsize=None)
def _noise_case(name):
    """(preds, target) fp32 on the CPU: 0.7 randn, some elements exactly +-1.0 and some beyond, and the fp64
    reference (value, dpreds, dtarget). Computed once and shared; never modified."""
    shape = _noise_shapes()[name]
    g = torch.Generator().manual_seed(NOISE_CASES.index(name) + 11)
    p, t = 0.7 * torch.randn(*shape, generator=g), 0.7 * torch.randn(*shape, generator=g)
    for x in (p, t):
        flat = x.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:max(8, flat.numel() // 16)]
        k = len(idx) // 4
        flat[idx[:k]] = 1.0
        flat[idx[k:2 * k]] = -1.0
        flat[idx[2 * k:3 * k]] = 1.5
        flat[idx[3 * k:]] = -1.25
    return (p, t) + _reference(p, t)


def _reference(p, t):
    from training.loss import SSIM
    pr, tr = p.double().requires_grad_(), t.double().requires_grad_()
    v = SSIM(data_range=2.0)(pr.clamp(-1, 1), tr.clamp(-1, 1))
    v.backward()
    return v.detach(), pr.grad, tr.grad


def _hip(p, t, both=False, noncontiguous=False):
    """SSIM(clamp=(-1, 1)) on the GPU with kernel_timer on: (value, dpreds, dtarget or None, region names)."""
    from training.loss import SSIM
    from torch_utils.ops import kernel_timer as kt
    if noncontiguous:
        pg = p.transpose(2, 3).contiguous().to(DEV).requires_grad_()
        pin = pg.transpose(2, 3)
        assert not pin.is_contiguous()
    else:
        pin = pg = p.to(DEV).requires_grad_()
    tg = t.to(DEV).requires_grad_(both)
    kt.enable(True)
    try:
        v = SSIM(data_range=2.0)(pin, tg, clamp=(-1, 1))
        v.backward()
        torch.cuda.synchronize()
        names = set(kt.summary())
    finally:
        kt.enable(False)
    dp = pg.grad.transpose(2, 3) if noncontiguous else pg.grad
    return v.detach().cpu(), dp.cpu(), tg.grad.cpu() if both else None, names


@pytest.mark.parametrize("name", NOISE_CASES)
def test_noise_cases(name):
    p, t, vr, dpr, dtr = _noise_case(name)
    both, nc = name == "ragged", name == "partial_tile"
    v, dp, dt, names = _hip(p, t, both=both, noncontiguous=nc)
    print(f"{name}: |value - ref| = {abs(float(v) - float(vr)):.3e}, rel(dpreds) = {_rel(dp, dpr):.3e}"
          + (f", rel(dtarget) = {_rel(dt, dtr):.3e}" if both else ""))
    assert {"ssim_fwd<f32>", "ssim_bwd<f32>"} <= names, names
    assert abs(float(v) - float(vr)) <= VALUE_TOL
    assert _rel(dp, dpr) <= GRAD_TOL
    if both:
        assert _rel(dt, dtr) <= GRAD_TOL
    # clamp backward: nothing passes beyond the bounds, the bounds themselves are inside (inclusive mask)
    beyond, at = p.abs() > 1, p.abs() == 1
    assert beyond.any() and at.any()
    assert (dp[beyond] == 0).all()
    assert ((dp[at] != 0) == (dpr[at] != 0)).all() and (dpr[at] != 0).any()
    # an element's rounding error scales with the largest terms of its sums, of the order of max |ref|
    assert float((dp[at].double() - dpr[at]).abs().max()) <= GRAD_TOL * float(dpr.abs().max())


def _cancellation_inputs(name):
    g = torch.Generator().manual_seed(5)
    if name == "smooth":
        y, x = torch.meshgrid(torch.arange(96.), torch.arange(96.), indexing="ij")
        img = torch.stack([0.5 * torch.sin(x / 7 + c) + 0.3 * torch.cos(y / 5 - c) for c in range(3)])[None]
        return img + 0.02 * torch.randn(img.shape, generator=g), img.clone()
    flat = torch.full((1, 1, 40, 40), 0.9)
    return flat + 0.01 * torch.randn(flat.shape, generator=g), flat


@pytest.mark.parametrize("name", ["smooth", "flat"])
def test_cancellation_cases(name):
    """epp - mp^2 cancels in fp32 for any formulation here, so the bound is taken from the torch fp32
    formulation's own error against fp64 on the CPU: 4x that error (22 taps summed in another order than
    121), and never less than the noise-case bound."""
    from training.loss import SSIM
    p, t = _cancellation_inputs(name)
    vr, dpr, _ = _reference(p, t)
    p32 = p.clone().requires_grad_()
    v32 = SSIM(data_range=2.0)(p32.clamp(-1, 1), t.clamp(-1, 1))
    v32.backward()
    v32 = v32.detach()
    v_tol = max(4 * abs(float(v32) - float(vr)), VALUE_TOL)
    g_tol = max(4 * _rel(p32.grad, dpr), GRAD_TOL)
    v, dp, _, _ = _hip(p, t)
    print(f"{name}: value err {abs(float(v) - float(vr)):.3e} (torch fp32 {abs(float(v32) - float(vr)):.3e}), "
          f"grad rel {_rel(dp, dpr):.3e} (torch fp32 {_rel(p32.grad, dpr):.3e})")
    assert abs(float(v) - float(vr)) <= v_tol
    assert _rel(dp, dpr) <= g_tol


def test_identical_inputs_give_one():
    from training.loss import SSIM
    g = torch.Generator().manual_seed(3)
    p = (0.7 * torch.randn(1, 3, 37, 53, generator=g)).to(DEV)
    v = SSIM(data_range=2.0)(p, p.clone(), clamp=(-1, 1))
    assert abs(float(v) - 1.0) <= 1e-6


def test_nan_in_preds_gives_nan():
    from training.loss import SSIM
    p, t = _noise_case("ragged")[:2]
    p = p.clone()
    p[1, 0, 20, 33] = float("nan")
    v = SSIM(data_range=2.0)(p.to(DEV), t.to(DEV), clamp=(-1, 1))
    assert torch.isnan(v)


def test_two_runs_agree_bitwise():
    p, t = _noise_case("tiles_plus_rest")[:2]
    a, b = _hip(p, t, both=True), _hip(p, t, both=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


WATCHED = ("aten.convolution", "aten._convolution", "aten.miopen_convolution", "aten.cudnn_convolution", "aten.clamp",
           "aten.reflection_pad2d")


class _Record(TorchDispatchMode):
    """Every watched aten op on a ROCm tensor (the recorder of tests/test_no_vendor_gemm_gpu.py, with the ops
    of the torch SSIM formulation)."""

    def __init__(self):
        super().__init__()
        self.hits = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if name.startswith(WATCHED) and any(isinstance(a, torch.Tensor) and a.is_cuda for a in args):
            self.hits.append(name)
        return func(*args, **(kwargs or {}))


def _loss_call(p, t, grad=True):
    """TotalLoss.calculate_ssim_loss, unbound, on a namespace holding the module: (value, region names)."""
    from training.loss import SSIM, TotalLoss
    from torch_utils.ops import kernel_timer as kt
    ns = types.SimpleNamespace(ssim_module=SSIM(data_range=2.0))
    gen = p.to(DEV).requires_grad_(grad)
    real = t.to(DEV)
    kt.enable(True)
    try:
        loss = TotalLoss.calculate_ssim_loss(ns, real, gen)
        if grad:
            loss.backward()
        torch.cuda.synchronize()
        names = set(kt.summary())
    finally:
        kt.enable(False)
    return loss.detach().cpu(), gen.grad, names


def test_loss_routes_to_the_kernels():
    p, t, vr, dpr, _ = _noise_case("ragged")
    rec = _Record()
    with rec:
        loss, grad, names = _loss_call(p, t)
    assert not rec.hits, rec.hits
    assert {"ssim_fwd<f32>", "ssim_bwd<f32>"} <= names, names
    assert abs(float(loss) - (1.0 - float(vr))) <= VALUE_TOL
    assert _rel(-grad, dpr) <= GRAD_TOL
    with torch.no_grad():
        loss, _, names = _loss_call(p, t, grad=False)
    assert names == {"ssim_fwd<f32>"}, names
    assert abs(float(loss) - (1.0 - float(vr))) <= VALUE_TOL


def test_loss_call_has_no_host_sync():
    from test_no_host_sync_gpu import _sync_watch
    from training.loss import SSIM, TotalLoss
    p, t = _noise_case("ragged")[:2]
    ns = types.SimpleNamespace(ssim_module=SSIM(data_range=2.0))
    gen, real = p.to(DEV).requires_grad_(), t.to(DEV)
    TotalLoss.calculate_ssim_loss(ns, real, gen).backward()      # warm: library and code objects loaded
    torch.cuda.synchronize()
    with _sync_watch() as hits:
        TotalLoss.calculate_ssim_loss(ns, real, gen).backward()
    torch.cuda.synchronize()
    assert not hits, hits


def _regions(fn):
    from torch_utils.ops import kernel_timer as kt
    kt.enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = set(kt.summary())
    finally:
        kt.enable(False)
    return out, names


def test_force_ref_takes_the_torch_formulation_and_agrees():
    from training.loss import SSIM
    from torch_utils.ops import decoder_ops
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")        # as training_loop.configure_backends
    p, t, vr, dpr, _ = _noise_case("partial_tile")
    v, dp, _, _ = _hip(p, t)
    pg, tg = p.to(DEV).requires_grad_(), t.to(DEV)
    decoder_ops.set_force_ref(True)
    try:
        vt, names = _regions(lambda: SSIM(data_range=2.0)(pg, tg, clamp=(-1, 1)))
        vt.backward()
    finally:
        decoder_ops.set_force_ref(False)
    assert not any(n.startswith("ssim_") for n in names), names
    assert abs(float(vt.detach()) - float(v)) <= VALUE_TOL
    assert _rel(pg.grad, dp) <= GRAD_TOL


def test_bf16_and_small_planes_stay_on_torch():
    from training.loss import SSIM
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    p, t = _noise_case("partial_tile")[:2]
    m = SSIM(data_range=2.0)
    v, names = _regions(lambda: m(p.to(DEV).bfloat16(), t.to(DEV).bfloat16(), clamp=(-1, 1)))
    assert v.dtype == torch.bfloat16 and not any(n.startswith("ssim_") for n in names), names
    _, names = _regions(lambda: m(p[..., :10, :10].to(DEV), t[..., :10, :10].to(DEV), clamp=(-1, 1)))
    assert not any(n.startswith("ssim_") for n in names), names
