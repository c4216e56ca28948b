"""torch_utils/ops/resize_det.py: F.interpolate's forward, and a backward that is the same linear map's adjoint
computed as a fixed-order gather (torch's GPU backward scatters with atomic adds and is not reproducible from run
to run). Reference: torch's own autograd of F.interpolate on the CPU in float64."""
import pytest
import torch
import torch.nn.functional as F

from torch_utils.ops import resize_det

# (H, W) -> size or scale: the discriminator's 256 -> 224 antialiased downsample and its upsamples from the
# equivariance scales, the latent's scale-factor downsample, an odd non-square case
CASES = [
    ((256, 256), dict(size=224, mode="bilinear", antialias=True)),
    ((256, 256), dict(size=224, mode="bicubic", antialias=True)),
    ((64, 64), dict(size=224, mode="bilinear")),
    ((192, 192), dict(size=224, mode="bicubic")),
    ((16, 16), dict(scale_factor=0.75, mode="bilinear")),
    ((16, 16), dict(scale_factor=0.25, mode="bilinear")),
    ((37, 53), dict(size=(29, 61), mode="bilinear", antialias=True)),
]


@pytest.mark.parametrize("shape,kw", CASES, ids=[f"{s[0]}x{s[1]}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for s, kw in CASES])
def test_forward_is_interpolate_and_backward_is_its_adjoint(shape, kw):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, *shape, generator=g)
    ref_kw = dict(kw, align_corners=False)
    xr = x.double().requires_grad_(True)
    yr = F.interpolate(xr, **ref_kw)
    dy = torch.randn(yr.shape, generator=g, dtype=torch.float64)
    yr.backward(dy)
    xt = x.clone().requires_grad_(True)
    y = resize_det.interpolate(xt, align_corners=False, **kw)
    assert torch.equal(y, F.interpolate(x, **ref_kw))           # the forward pass is F.interpolate itself
    y.backward(dy.float())
    # fp32 products and sums of at most a few dozen terms against float64: 1e-5 of the largest gradient
    err = float((xt.grad.double() - xr.grad).abs().max() / xr.grad.abs().max())
    assert err < 1e-5, err


def test_no_gradient_needed_is_plain_interpolate():
    x = torch.randn(1, 2, 8, 8)
    y = resize_det.interpolate(x, 5, mode="bilinear", antialias=True)
    assert y.grad_fn is None and torch.equal(y, F.interpolate(x, 5, mode="bilinear", align_corners=False, antialias=True))
    with torch.no_grad():
        z = resize_det.interpolate(x.requires_grad_(True), 5, mode="bicubic")
    assert z.grad_fn is None


def test_backward_is_bitwise_repeatable():
    """The same gradient twice: the gather sums in a fixed order."""
    x = torch.randn(2, 3, 40, 40, requires_grad=True)
    dy = torch.randn(2, 3, 35, 35)
    outs = []
    for _ in range(2):
        x.grad = None
        resize_det.interpolate(x, 35, mode="bilinear", antialias=True).backward(dy)
        outs.append(x.grad.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gpu_backward_matches_cpu_and_repeats(dtype):
    """On the GPU: the 256 -> 224 antialiased case against the CPU float64 gradient, and twice bit for bit."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 256, 256, generator=g)
    dy = torch.randn(4, 3, 224, 224, generator=g)
    xr = x.double().requires_grad_(True)
    F.interpolate(xr, 224, mode="bilinear", align_corners=False, antialias=True).backward(dy.double())
    outs = []
    for _ in range(2):
        xg = x.cuda().to(dtype).requires_grad_(True)
        resize_det.interpolate(xg, 224, mode="bilinear", antialias=True).backward(dy.cuda().to(dtype))
        outs.append(xg.grad.float().cpu())
    assert torch.equal(outs[0], outs[1])
    # fp32: as on the CPU; bf16: inputs and the result rounded to 8 bits of mantissa (2^-8 each, three roundings)
    tol = 1e-5 if dtype == torch.float32 else 3 * 2.0 ** -8
    err = float((outs[0].double() - xr.grad).abs().max() / xr.grad.abs().max())
    assert err < tol, err
