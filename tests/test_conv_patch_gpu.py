"""The patch-staged form of the f32x6 3x3 conv (csrc/conv.hip conv3x3_patch_kernel; vfm_conv3x3_nhwc_f32_form
form 2) against the tiled kernel (form 1) and fp64 torch: the patch form keeps the tiled kernel's K order, MFMA
slot mapping, term order and accumulators, so its outputs are bit-identical; against fp64 F.conv2d it meets the
bounds tests/test_vgg_gpu.py applies to the tiled kernel (3e-6 of max |ref|, and for the forward layers within
2x (+1e-7) of the exact-fp32 torch conv's own error). Inputs span 1e-3 .. 1e3 in magnitude with exact zeros.
Routing: planes that are no multiple of the 16 x 16 patch give VFM_NO_KERNEL for form 2 and run the tiled
kernel under auto; the VFM_CONV_PATCH switch (vgg_hip.CONV_PATCH) does not change the VGG16 taps or the input
gradient by a bit."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.678
PAD = 1024          # floats before and after the output (keeps it 16-B aligned)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _inputs(B, H, W, Cin, Cout, seed):
    from torch_utils.ops import vgg_hip
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g, device=DEV)
    x = x * torch.pow(10.0, 6 * torch.rand(B, H, W, Cin, generator=g, device=DEV) - 3)     # 1e-3 .. 1e3
    x = torch.where(torch.rand(B, H, W, Cin, generator=g, device=DEV) < 0.1, torch.zeros_like(x), x).contiguous()
    w = torch.randn(Cout, Cin, 3, 3, generator=g, device=DEV) * (9 * Cin) ** -0.5
    bias = torch.randn(Cout, generator=g, device=DEV)
    mask = torch.randn(B, H, W, Cout, generator=g, device=DEV)
    w2d = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)                                       # tap-major
    pieces = vgg_hip.split_weight(vgg_hip.chunk_major(w2d, Cin).contiguous(), 3)
    return x, w, bias, mask, pieces


def _run(form, x, pieces, bias, mask, relu, Cout):
    """(return code, output view, whole sentinel-filled buffer) of one call of the C entry."""
    from torch_utils import custom_ops
    lib = custom_ops.get_native()
    B, H, W, Cin = x.shape
    n = B * H * W * Cout
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[PAD:PAD + n].view(B, H, W, Cout)
    rc = lib.vfm_conv3x3_nhwc_f32_form(x.data_ptr(), pieces.data_ptr(), custom_ops.VFM_F32, pieces.shape[2],
                                       custom_ops.ptr(bias), custom_ops.ptr(mask), out.data_ptr(), B, H, W, Cin, Cout,
                                       int(relu), custom_ops.stream_ptr(x.device), form)
    torch.cuda.synchronize()
    return rc, out, buf


def _sentinel_intact(buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


# one patch per image (every halo side is the border), one chunk; interior seams both ways, non-square, two
# chunks, two Cout tiles; the data-gradient form (mask, no bias, no ReLU), four chunks
@pytest.mark.parametrize("B,H,W,Cin,Cout,fwd", [(2, 16, 16, 32, 128, True), (1, 32, 48, 64, 256, True),
                                                (3, 16, 16, 128, 128, False)])
def test_patch_form_matches_tiled_and_fp64(B, H, W, Cin, Cout, fwd):
    x, w, bias, mask, pieces = _inputs(B, H, W, Cin, Cout, seed=H * W + Cin)
    args = (x, pieces, bias, None, True, Cout) if fwd else (x, pieces, None, mask, False, Cout)
    rc1, y1, buf1 = _run(1, *args)
    rc2, y2, buf2 = _run(2, *args)
    assert rc1 == 0 and rc2 == 0, (rc1, rc2)
    assert _sentinel_intact(buf1) and _sentinel_intact(buf2)
    assert not bool((y2 == SENTINEL).any())
    assert torch.equal(y2, y1)
    xn = x.permute(0, 3, 1, 2)
    if fwd:
        ref = F.conv2d(xn.double(), w.double(), bias.double(), padding=1).relu()
        with torch.backends.cudnn.flags(enabled=False):      # torch's direct fp32 conv (exact products)
            yt = F.conv2d(xn, w, bias, padding=1).relu()
    else:
        ref = F.conv2d(xn.double(), w.double(), None, padding=1) * (mask.permute(0, 3, 1, 2) > 0)
    e = _rel(y2.permute(0, 3, 1, 2), ref)
    print(f"patch form vs fp64: {e:.3e}" + (f" (torch fp32 conv: {_rel(yt, ref):.3e})" if fwd else ""))
    assert e < 3e-6, e
    if fwd:
        assert e <= 2 * _rel(yt, ref) + 1e-7, (e, _rel(yt, ref))


@pytest.mark.parametrize("HW", [24, 8])
def test_patch_form_routing(HW):
    """Planes that are no multiple of the patch: form 2 has no kernel, auto runs the tiled kernel."""
    from torch_utils import custom_ops
    x, w, bias, mask, pieces = _inputs(1, HW, HW, 64, 128, seed=HW)
    rc2, _, buf2 = _run(2, x, pieces, bias, None, True, 128)
    assert rc2 == custom_ops.VFM_NO_KERNEL
    assert bool((buf2 == SENTINEL).all())
    rc0, y0, buf0 = _run(0, x, pieces, bias, None, True, 128)
    rc1, y1, _ = _run(1, x, pieces, bias, None, True, 128)
    assert rc0 == 0 and rc1 == 0
    assert _sentinel_intact(buf0)
    assert torch.equal(y0, y1)


def test_vgg16_taps_pair_same_with_and_without_patch_form():
    """The VGG16 tap stack (32^2 and 16^2 planes take the patch form where auto routes it) with the switch at
    its default against the tiled kernel forced: taps and input gradient bit-identical."""
    from training.lpips import vgg16
    from torch_utils.ops import vgg_hip
    assert vgg_hip.CONV_PATCH is True
    net = vgg16(pretrained=False).to(DEV)
    convs = [m for k in range(1, 6) for m in getattr(net, f"slice{k}") if isinstance(m, torch.nn.Conv2d)]
    g = torch.Generator(device=DEV).manual_seed(7)
    x0 = torch.randn(2, 3, 32, 32, generator=g, device=DEV).requires_grad_(True)
    x1 = torch.randn(2, 3, 32, 32, generator=g, device=DEV)
    res = {}
    try:
        for patch in (True, False):
            vgg_hip.CONV_PATCH = patch
            t0, t1 = vgg_hip.vgg16_taps_pair(x0, x1, convs)
            if patch:
                gs = [torch.randn(o.shape, generator=g, device=DEV) for o in t0]
            gx, = torch.autograd.grad(list(t0), [x0], gs)
            res[patch] = (list(t0) + list(t1), gx)
    finally:
        vgg_hip.CONV_PATCH = True
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b)
    assert torch.equal(res[True][1], res[False][1])
