"""SSIM loss: the identity the HIP kernels rest on, their C ABI's argument checks, and the timer names.

training.loss.SSIM (the torchmetrics StructuralSimilarityIndexMeasure restatement) reflect-pads by 5,
filters with the 121-tap window, drops a 5-wide border and takes the mean; the kept windows never leave
the image, so the result equals the mean of the VALID separable correlation of the unpadded planes,
which is what csrc/ssim.hip computes. No GPU needed."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT  # noqa: F401  (sys.path)

SHAPES = [(2, 3, 11, 11), (1, 3, 12, 37), (2, 1, 45, 70)]


def valid_window_ssim(p, t, data_range=2.0, size=11, sigma=1.5, k1=0.01, k2=0.03):
    """No padding; rows then columns with the 1-d Gaussian (11 + 11 taps); mean of the valid map."""
    from training.loss import _gaussian_window
    g = _gaussian_window(size, sigma, p.device, p.dtype)
    B, C, H, W = p.shape

    def G(x):
        x = x.reshape(B * C, 1, H, W)
        x = F.conv2d(x, g.view(1, 1, 1, size))
        return F.conv2d(x, g.view(1, 1, size, 1))

    mp, mt, epp, ett, ept = G(p), G(t), G(p * p), G(t * t), G(p * t)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    spp, stt, spt = epp - mp * mp, ett - mt * mt, ept - mp * mt
    return (((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2))).mean()


def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.7 * torch.randn(*shape, generator=g, dtype=torch.float64),
            0.7 * torch.randn(*shape, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("shape", SHAPES)
def test_ssim_equals_valid_window_formulation(shape):
    from training.loss import SSIM
    p, t = _images(shape, sum(shape))
    assert abs(float(SSIM(data_range=2.0)(p, t)) - float(valid_window_ssim(p, t))) <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_clamp_keyword_equals_clamping_beforehand(shape):
    from training.loss import SSIM
    p, t = _images(shape, 7 + sum(shape))
    m = SSIM(data_range=2.0)
    assert (p.abs() > 1).any() and (t.abs() > 1).any()
    a, b = m(p, t, clamp=(-1, 1)), m(p.clamp(-1, 1), t.clamp(-1, 1))
    assert float(a) == float(b)
    assert float(a) != float(m(p, t))


def _lib():
    import torch_utils.custom_ops as co
    return co.get_native()


def test_argument_validation_without_gpu():
    """Invalid arguments are rejected before any device work: VFM_ERR_ARGS (-2) for null pointers and planes
    smaller than the window, "no kernel" (-1) for a window length other than 11."""
    lib = _lib()
    p = ctypes.c_void_p(64)
    taps = (ctypes.c_float * 11)(*([1 / 11] * 11))
    c = (1e-4, 9e-4, -1.0, 1.0, 1)
    assert lib.vfm_ssim_fwd(None, p, p, p, taps, 11, *c, 1, 3, 16, 16, None) == -2
    assert lib.vfm_ssim_fwd(p, p, p, None, taps, 11, *c, 1, 3, 16, 16, None) == -2
    assert lib.vfm_ssim_fwd(p, p, p, p, None, 11, *c, 1, 3, 16, 16, None) == -2
    assert lib.vfm_ssim_fwd(p, p, p, p, taps, 11, *c, 1, 3, 10, 16, None) == -2
    assert lib.vfm_ssim_fwd(p, p, p, p, taps, 11, *c, 1, 3, 16, 10, None) == -2
    assert lib.vfm_ssim_fwd(p, p, p, p, taps, 11, *c, 0, 3, 16, 16, None) == -2
    assert lib.vfm_ssim_fwd(p, p, p, p, taps, 7, *c, 1, 3, 16, 16, None) == -1
    assert lib.vfm_ssim_bwd(p, None, p, p, taps, 11, *c, 1, 3, 16, 16, None) == -2
    assert lib.vfm_ssim_bwd(p, p, None, p, taps, 11, *c, 1, 3, 16, 16, None) == -2
    assert lib.vfm_ssim_bwd(p, p, p, p, taps, 11, *c, 1, 3, 10, 16, None) == -2
    assert lib.vfm_ssim_bwd(p, p, p, p, taps, 11, *c, 1, 0, 16, 16, None) == -2
    assert lib.vfm_ssim_bwd(p, p, p, p, taps, 7, *c, 1, 3, 16, 16, None) == -1


def test_partials_follow_the_tile_constants():
    """One partial per (plane, TILE_H x TILE_W tile of the (H-10) x (W-10) map): the Python constants the GPU
    tests size their ragged case from are the kernels'; a grid that does not fit is refused."""
    from torch_utils.ops import ssim_hip
    lib = _lib()
    th, tw = ssim_hip.TILE_H, ssim_hip.TILE_W
    assert lib.vfm_ssim_fwd_partials(1, 1, 11, 11) == 1
    assert lib.vfm_ssim_fwd_partials(1, 1, 10 + th, 10 + tw) == 1
    assert lib.vfm_ssim_fwd_partials(1, 1, 11 + th, 10 + tw) == 2
    assert lib.vfm_ssim_fwd_partials(1, 1, 10 + th, 11 + tw) == 2
    assert lib.vfm_ssim_fwd_partials(2, 3, 10 + 2 * th + 3, 10 + 3 * tw + 1) == 6 * 3 * 4
    assert lib.vfm_ssim_fwd_partials(1, 1, 10, 64) == -2
    assert lib.vfm_ssim_fwd_partials(1 << 20, 1 << 10, 4096, 4096) == -2


def test_host_taps_are_the_gaussian_window():
    from torch_utils.ops import ssim_hip
    from training.loss import _gaussian_window
    taps = ssim_hip.gaussian_taps(11, 1.5)
    ref = _gaussian_window(11, 1.5, "cpu", torch.float64).float()
    assert list(taps) == ref.tolist()
    assert ssim_hip.gaussian_taps(11, 1.5) is taps


def test_timer_regions_have_rocprof_names():
    from torch_utils.ops import kernel_timer
    for region, kernel in (("ssim_fwd<f32>", "ssim_fwd"), ("ssim_bwd<f32>", "ssim_bwd")):
        pat = kernel_timer.rocprof_name(region)
        assert pat is not None
        assert kernel_timer.roc_match(pat, f"(anonymous namespace)::{kernel}(float const*, float const*)")
    assert not kernel_timer.roc_match(kernel_timer.rocprof_name("ssim_fwd<f32>"), "(anonymous namespace)::ssim_finish()")
