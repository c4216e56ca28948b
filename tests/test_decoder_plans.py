"""The launch plans tests/test_decoder_guard_gpu.py relies on, through the host-side sizing entries (no GPU: the
library loads without one, see tests/test_native_lib.py). The case tables are the GPU file's own: a planner change
that moves a case off the branch it was chosen for fails here, on a CPU-only run, as well as there."""
import pytest

import test_decoder_guard_gpu as G
from torch_utils import custom_ops

NO_KERNEL = custom_ops.VFM_NO_KERNEL


@pytest.fixture(scope="module")
def lib():
    return custom_ops.get_native()


def _dwr_plan(B, C, H, W):
    """csrc/decoder.hip dwr_plan restated: (band height, bands per plane, waves per channel)."""
    R = 64 // (W // 4)
    BH = 64
    while BH > 8 and BH // 2 >= H:
        BH //= 2
    while True:
        nb = -(-H // BH)
        wpc = -(-B * nb // R)
        if BH <= 8 or C * wpc >= 16384:
            return BH, nb, wpc
        BH //= 2


def test_tile_kernel_partial_slots(lib):
    for shape, pad, _, tiles in G.DW_TILE:
        for K in G.KS:
            p = (K - 1) // 2 if pad is None else pad
            if shape[2] + 2 * p - K + 1 > 0:
                assert lib.vfm_dwconv2d_bwd_weight_tiles(*shape, K, p) == tiles, (shape, K)


def test_row_kernel_band_height_8(lib):
    for shape, wpc in G.DW_ROW8:
        assert _dwr_plan(*shape) == (8, -(-shape[2] // 8), wpc)
        for K in G.KS:
            assert lib.vfm_dwconv2d_bwd_weight_tiles(*shape, K, (K - 1) // 2) == wpc, (shape, K)


def test_row_kernel_tall_bands(lib):
    """C * wpc >= 16384 at the wanted band height, a partial last band and a last wave with dead row groups."""
    for shape, BH, nb, wpc in G.DW_TALL:
        B, C, H, W = shape
        assert _dwr_plan(*shape) == (BH, nb, wpc)
        assert C * wpc >= 16384 and H % BH != 0 and (B * nb) % (64 // (W // 4)) != 0
        for K in G.KS:
            assert lib.vfm_dwconv2d_bwd_weight_tiles(*shape, K, (K - 1) // 2) == wpc, (shape, K)


def test_mfma_forward_units(lib):
    for shape, units in G.DWM_FWD:
        for K in G.KS:
            assert lib.vfm_dwconv2d_fwd_mfma_units(*shape, K, (K - 1) // 2) == units, (shape, K)
    for (B, C, H, W, _), units in G.GN_STATS:
        assert lib.vfm_dwconv2d_fwd_mfma_units(B, C, H, W, 7, 3) == units
        assert units % (B * C) == 0


def test_mfma_forward_last_group_is_short():
    """The shapes named for it: 16-row blocks do not fill the last group of rb = 4."""
    for (B, C, H, W), _ in G.DWM_FWD[2:]:
        rows16 = -(-H // 16)
        assert rows16 > 4 and rows16 % 4 != 0


def test_mfma_weight_gradient_tiles(lib):
    for shape, tiles in G.DWM_WGRAD:
        for K in G.KS:
            assert lib.vfm_dwconv2d_bwd_weight_mfma_tiles(*shape, K, (K - 1) // 2) == tiles, (shape, K)
    for (B, C, H, W), tiles in G.DWM_WGRAD[2:]:           # per > 1 with a last wave of fewer bands
        nb = B * -(-H // 32) * (W // (64 if W % 64 == 0 else 16))
        per = -(-nb // min(nb, -(-16384 // C)))
        assert per > 1 and -(-nb // per) == tiles and nb % per != 0, (nb, per)


def test_group_norm_stats_blocks():
    """gn_apply splits a group over blocks of 2048 chunks: the first case has a partial second block."""
    (B, C, H, W, Gr), _ = G.GN_STATS[0]
    chunks = (C // Gr) * H * W // 8
    assert 2048 < chunks < 4096
    (B, C, H, W, Gr), _ = G.GN_STATS[2]
    assert C // Gr > 128                                   # GN_FLAT_MAX: the one-block-per-group form


def test_channel_rms_norm_rows(lib):
    for (B, C, P), rows in G.RMS_SHAPES:
        assert lib.vfm_channel_rms_norm_rows(B, C, P) == rows == B * -(-P // 32)


def test_torgb_splits(lib):
    for (B, C, P, O), splits in G.TORGB_SHAPES:
        assert lib.vfm_torgb_bwd_splits(B, C, P) == splits


@pytest.mark.parametrize("args", [(1, 3, 16, 24, 7, 3),      # W % 16 != 0
                                  (1, 3, 16, 16, 9, 4),      # K = 9
                                  (1, 3, 16, 16, 7, 2),      # pad != (K - 1) / 2
                                  (1, 3, 16, 16, 4, 1)])     # even K
def test_mfma_entries_decline(lib, args):
    assert lib.vfm_dwconv2d_fwd_mfma_units(*args) == NO_KERNEL
    assert lib.vfm_dwconv2d_bwd_weight_mfma_tiles(*args) == NO_KERNEL
