"""Guard bands around the decoder kernel family (csrc/decoder.hip, dwconv_mfma.hip, rmsnorm.hip, torgb.hip,
posterior.hip) through the C ABI (custom_ops.get_native()): no stray reads that reach a stored value, no stray
writes, no unwritten output or workspace element, and fp64 parity (tests/decoder_refs.py) on the launch-plan
branches the op-level tests never leave their small-problem side of.

These entries take dense tensors, so every view is dense with its base 16 bytes past a 512-byte boundary
(tests/guard_bands.py); every input is embedded in NaN, every output and workspace is pre-filled with NaN and
embedded in a finite sentinel, and a workspace has exactly the element count its sizing entry returns. Every case
asserts, in this order: return code 0 (not VFM_NO_KERNEL for the MFMA entries); after one synchronize every guard
intact, inputs included; no NaN in any output or workspace element; parity against the fp64 restatement.

The case tables below name the plan values (band height, waves per channel, units, tiles) each shape was chosen
for; tests/test_decoder_plans.py asserts the same tables on the CPU through the host-side sizing entries.

Tolerances are those the existing test of each kernel states, here against fp64:
  tests/test_decoder_gpu.py         2e-5 of max |ref| for fp32 I/O, 1.5e-2 for bf16 / fp16, four times that on
                                    gradients; the MFMA weight gradient and the noise-strength dot 1e-5; GroupNorm
                                    from the dwconv's statistics 2e-5 (fp32 out)
  tests/test_style_rmsnorm_gpu.py   channel RMS norm 2e-5 forward, 1e-4 on gradients
  posterior (test_decoder_gpu.py)   1e-6 on z and kl, 1e-5 on the moment gradients
Statistics the kernels hand on (GroupNorm mean / rstd, the dwconv's merged per-wave partials) are fp32 sums about a
shift: 2e-5 of max(|mean|, std) on means, 2e-5 relative on rstd / of max on variances. The channel RMS norm's clamped
column (1 / 1e-12) is compared on its own, so that its 1e12 does not set the scale for every other column.

Every case prints its measured error next to its bound. Those bounds were set against fp32 torch; measured on an
MI355X against fp64, every shape here meets them as stated and none needed a bound derived from the torch fp32
formulation's own error: the largest fp32 errors are 8.0e-7 of the 2e-5 (GroupNorm from the dwconv's statistics),
3.5e-7 of the 8e-5 on gradients, 2.0e-7 of the posterior's 1e-6 (kl) and 1.6e-7 of the MFMA weight gradient's
1e-5; the largest bf16 / fp16 error is 3.6e-3 of the 1.5e-2 (one output rounding)."""
import ctypes

import pytest
import torch

import decoder_refs as R
import guard_bands as gb
from torch_utils import custom_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NO_KERNEL, ERR_ARGS = custom_ops.VFM_NO_KERNEL, -2
_lib = custom_ops.get_native()

# ------------------------------------------------------------------------------------------------------------------
# Case tables (plain data: tests/test_decoder_plans.py imports them). Shapes are (B, C, H, W).

KS = (3, 5, 7)

# vfm_dwconv2d_fwd_res, LDS-tile kernel (shapes the row-streaming plan rejects): (shape, pad or None = (K-1)/2, bias,
# weight-gradient partial slots = column tiles x samples)
DW_TILE = [((2, 5, 13, 9), None, True, 2), ((1, 2, 1, 5), None, True, 1), ((1, 4, 64, 70), None, True, 2),
           ((2, 4, 12, 20), 0, False, 2)]
# row-streaming kernel, band height 8: (shape, waves per channel)
DW_ROW8 = [((2, 8, 16, 16), 1),          # 4 units in 16 row groups
           ((5, 2, 8, 16), 1),           # 5 units for 16 row groups
           ((1, 3, 300, 64), 10)]        # 38 bands, 4 per wave: last band 4 rows, last wave 2 of 4 units
# row-streaming kernel, tall bands: (shape, band height, bands per plane, waves per channel)
DW_TALL = [((5, 8192, 17, 32), 16, 2, 2),    # last band 1 row, 10 units in 16 groups
           ((5, 8192, 33, 32), 32, 2, 2),
           ((1, 16384, 65, 16), 64, 2, 1)]   # 2 units in 16 groups
# vfm_dwconv2d_fwd_mfma_nz / _gs: (shape, units)
DWM_FWD = [((1, 3, 5, 16), 3),           # one partial block
           ((2, 3, 33, 48), 18),         # XW 16, rb 3
           ((1, 3, 72, 16), 6),          # rows16 5, last group one block of 8 rows
           ((2, 2, 80, 64), 8),          # XW 64, last group one block
           ((1, 2, 65, 128), 8)]         # two column strips, last block one row
# vfm_dwconv2d_bwd_weight_mfma: (shape, tiles)
DWM_WGRAD = [((3, 1, 16, 16), 3),        # 3 waves: the last block has one wave
             ((1, 3, 72, 16), 3),        # H % 32 != 0
             ((3, 2048, 16, 48), 5),     # nb 9, per 2: last wave one band, XW 16
             ((3, 2048, 16, 192), 5),    # the same with XW 64
             ((1, 4096, 33, 80), 4)]     # nb 10, per 3: last wave one band, H % 32 != 0
# GroupNorm: (B, C, H, W, G)
GN_SHAPES = [(2, 8, 4, 4, 1), (1, 16, 24, 24, 4), (2, 12, 5, 7, 3), (1, 512, 16, 16, 2), (2, 8, 1, 1, 2)]
GN_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (F16, F16)]
# GroupNorm from the dwconv's statistics: (B, C, H, W, G), dwconv units
GN_STATS = [((1, 10, 64, 64, 2), 10),    # 2560 chunks per group: two gridDim.y blocks, the last one partial
            ((2, 6, 16, 48, 2), 36),     # one block
            ((1, 256, 16, 16, 1), 256)]  # more than 128 channels per group: gn_fwd with stats
ROW_SHAPES = [(1, 3, 8), (3, 5, 520), (2, 40, 1000)]        # (B, O, P)
LSR_PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)]      # (y, x_in): LSR_DISPATCH
BLUR_SHAPES = [((1, 4, 1, 1), 2), ((1, 12, 5, 7), 2), ((1, 4, 3, 8), 2), ((1, 3, 72, 136), 1), ((1, 4, 136, 16), 2)]
BLUR_TAPS = [[1, 1], [1, 3, 3, 1], [1, 7, 21, 35, 35, 21, 7, 1]]
# channel RMS norm: (B, C, P), rows of gpart
RMS_SHAPES = [((2, 40, 35), 4), ((1, 300, 64), 2), ((3, 256, 1024), 96)]
# ToRGB: (B, C, P, O), pixel splits
TORGB_SHAPES = [((2, 16, 8, 4), 1), ((3, 256, 768, 1), 2), ((2, 512, 64, 3), 1)]
POSTERIOR_SHAPES = [(3, 8, 25), (4, 32, 256)]               # (B, C, P)


def _ks(i):
    """K in {3, 5, 7} on the first shape of a group, 7 elsewhere."""
    return KS if i == 0 else (7,)


def _shape_k(table):
    return [(row, K) for i, row in enumerate(table) for K in _ks(i)]


def _id(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    if isinstance(v, (tuple, list)):
        return "-".join(_id(x) for x in v)
    return str(v)


# ------------------------------------------------------------------------------------------------------------------
# Harness

def _tol(dt):
    return 2e-5 if dt == F32 else 1.5e-2


def _p(t):
    return None if t is None else t.data_ptr()


def _code(dt):
    return custom_ops.DTYPE_CODES[dt]


def _st():
    return custom_ops.stream_ptr()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=DEV)


class Case:
    """The operands of one guarded call (or of a chain of calls: an output may feed the next entry)."""

    def __init__(self):
        self.guards, self.outs = [], []

    def inp(self, name, t):
        if t is None:
            return None
        v, buf = gb.embed(t.contiguous(), fill=gb.POISON)
        assert v.data_ptr() % 512 == 16 and v.is_contiguous()
        self.guards.append((name, v, buf, gb.POISON))
        return v

    def out(self, name, shape, dtype=F32):
        v, buf = gb.embed(torch.full(tuple(shape), gb.POISON, dtype=dtype, device=DEV), fill=gb.SENTINEL)
        assert v.data_ptr() % 512 == 16 and v.is_contiguous()
        self.guards.append((name, v, buf, gb.SENTINEL))
        self.outs.append((name, v))
        return v

    def check(self, written=True):
        """Guards first (after one synchronize), then every output: whole (written) or untouched."""
        torch.cuda.synchronize()
        for name, v, buf, fill in self.guards:
            assert gb.intact(v, buf, fill), f"{name}: " + gb.describe(v, buf, fill)
        for name, v in self.outs:
            nan = torch.isnan(v)
            if written:
                assert not nan.any(), f"{name}: {int(nan.sum())} of {v.numel()} NaN (unwritten or poisoned), " \
                                      f"first at flat index {int(nan.flatten().nonzero()[0])}"
            else:
                assert bool(nan.all()), f"{name}: written by a call that was to decline"


def _err(out, ref):
    return float((out.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _check(tag, out, ref, tol):
    assert out.shape == ref.shape, (tag, out.shape, ref.shape)
    e = _err(out, ref)
    print(f"{tag}: err {e:.3e} of max (tol {tol:.1e})")
    assert e < tol, (tag, e, tol)


def _check_stats(tag, mean, rstd, mref, rref):
    """fp32 statistics about a shift: means within 2e-5 of max(|mean|, std), rstd within 2e-5 relative."""
    scale = float(torch.maximum(mref.abs(), 1.0 / rref).max())
    em = float((mean.double() - mref).abs().max()) / scale
    er = float(((rstd.double() - rref).abs() / rref).max())
    print(f"{tag}: mean err {em:.3e} of max(|mean|, std), rstd rel err {er:.3e} (tol 2e-5)")
    assert em < 2e-5 and er < 2e-5, (tag, em, er)


# ------------------------------------------------------------------------------------------------------------------
# Depthwise conv: vfm_dwconv2d_fwd_res (LDS-tile and row-streaming kernels), vfm_dwconv2d_bwd_weight + reduce

def _dw_fwd(shape, K, dt, *, pad=None, bias=True, noise=False, res=False, flip=False, seed=0, tag="dwconv"):
    B, C, H, W = shape
    pad = (K - 1) // 2 if pad is None else pad
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    g = _gen(1000 * K + H + W + seed)
    x = _randn(g, B, C, H, W).to(dt)
    w = _randn(g, C, K, K) * 0.2
    b = _randn(g, C) * 0.1 if bias else None
    nz = _randn(g, Ho, Wo) if noise else None
    rs = _randn(g, B, C, Ho, Wo).to(dt) if res else None
    c = Case()
    xv, wv, bv, nv, rv = (c.inp(n, t) for n, t in (("x", x), ("w", w), ("bias", b), ("noise", nz), ("res", rs)))
    y = c.out("y", (B, C, Ho, Wo), dt)
    rc = _lib.vfm_dwconv2d_fwd_res(_p(xv), _p(wv), _p(bv), _p(nv), _p(rv), _p(y), _code(dt), B, C, H, W, K, pad,
                                   int(flip), _st())
    assert rc == 0, rc
    c.check()
    _check(tag, y, R.dwconv(x, w, b, nz, rs, pad, flip), (4 if flip else 1) * _tol(dt))


def _dw_wgrad(shape, K, dt, *, pad=None, tiles=None, null=None, seed=0, tag="dwconv wgrad"):
    """vfm_dwconv2d_bwd_weight into a partial buffer of exactly vfm_dwconv2d_bwd_weight_tiles slots, then
    vfm_dwconv2d_wgrad_reduce (null: 'dw' or 'db' passed as a null pointer)."""
    B, C, H, W = shape
    pad = (K - 1) // 2 if pad is None else pad
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    g = _gen(2000 * K + H + W + seed)
    x, dy = _randn(g, B, C, H, W).to(dt), _randn(g, B, C, Ho, Wo).to(dt)
    n = _lib.vfm_dwconv2d_bwd_weight_tiles(B, C, H, W, K, pad)
    assert n > 0 and (tiles is None or n == tiles), (n, tiles)
    c = Case()
    xv, dv = c.inp("x", x), c.inp("dy", dy)
    part = c.out("partial", (n, C, K * K + 1))
    rc = _lib.vfm_dwconv2d_bwd_weight(_p(xv), _p(dv), _p(part), _code(dt), B, C, H, W, K, pad, _st())
    assert rc == 0, rc
    c.check()
    _reduce_and_check(c, part, x, dy, K, pad, 4 * _tol(dt), null, tag)


def _reduce_and_check(c, part, x, dy, K, pad, tol, null, tag):
    C = part.shape[1]
    dw = None if null == "dw" else c.out("dw", (C, K, K))
    db = None if null == "db" else c.out("db", (C,))
    rc = _lib.vfm_dwconv2d_wgrad_reduce(_p(part), _p(dw), _p(db), part.shape[0], C, K * K, _st())
    assert rc == 0, rc
    c.check()
    dwr, dbr = R.dwconv_wgrad(x, dy, K, pad)
    if dw is not None:
        _check(tag + " dw", dw, dwr, tol)
    if db is not None:
        _check(tag + " db", db, dbr, tol)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=_id)
@pytest.mark.parametrize("row,K", _shape_k(DW_TILE), ids=_id)
def test_dwconv_tile_kernel(row, K, dt):
    """The LDS-tile kernel: ragged widths, a one-row plane, valid padding without bias; with and without noise,
    with and without res, taps as stored and rotated."""
    shape, pad, bias, tiles = row
    for i in range(8):
        noise, res, flip = bool(i & 1), bool(i & 2), bool(i & 4)
        _dw_fwd(shape, K, dt, pad=pad, bias=bias, noise=noise, res=res, flip=flip, seed=i,
                tag=f"tile {shape} K{K} {_id(dt)} noise={noise} res={res} flip={flip}")
    _dw_wgrad(shape, K, dt, pad=pad, tiles=tiles, tag=f"tile wgrad {shape} K{K} {_id(dt)}")


@pytest.mark.parametrize("dt", [F32, F16], ids=_id)
@pytest.mark.parametrize("row,K", _shape_k(DW_ROW8), ids=_id)
def test_dwconv_row_kernel_bh8(row, K, dt):
    shape, wpc = row
    tag = f"row8 {shape} K{K} {_id(dt)}"
    _dw_fwd(shape, K, dt, noise=True, tag=tag + " fwd")
    _dw_fwd(shape, K, dt, bias=False, res=True, flip=True, tag=tag + " flip+res")
    _dw_wgrad(shape, K, dt, tiles=wpc, tag=tag + " wgrad")


TALL = [(row, K, dt) for i, row in enumerate(DW_TALL) for K in _ks(i) for dt in ((F16, F32) if i == 0 else (F16,))]


@pytest.mark.parametrize("form", ["fwd", "flip_res", "wgrad"])
@pytest.mark.parametrize("row,K,dt", TALL, ids=_id)
def test_dwconv_row_kernel_tall_bands(row, K, dt, form):
    """Band heights 16 / 32 / 64 (C * wpc >= 16384 keeps dwr_plan from halving further): a partial last band,
    several samples per wave, dead row groups in the last wave. vfm_dwconv2d_bwd_weight_tiles == wpc pins the plan
    branch the shape was chosen for."""
    shape, BH, nb, wpc = row
    assert _lib.vfm_dwconv2d_bwd_weight_tiles(*shape, K, (K - 1) // 2) == wpc
    assert shape[1] * wpc >= 16384 and shape[2] % BH != 0 and -(-shape[2] // BH) == nb
    tag = f"tall BH{BH} {shape} K{K} {_id(dt)} {form}"
    if form == "fwd":
        _dw_fwd(shape, K, dt, noise=True, tag=tag)
    elif form == "flip_res":
        _dw_fwd(shape, K, dt, bias=False, res=True, flip=True, tag=tag)
    else:
        _dw_wgrad(shape, K, dt, tiles=wpc, tag=tag)


@pytest.mark.parametrize("null", ["dw", "db"])
def test_dwconv_wgrad_reduce_null_output(null):
    _dw_wgrad((2, 5, 13, 9), 5, F32, null=null, tag=f"wgrad reduce without {null}")


# ------------------------------------------------------------------------------------------------------------------
# Banded-MFMA depthwise conv (bf16): vfm_dwconv2d_fwd_mfma_nz / _gs, vfm_dwconv2d_bwd_weight_mfma

def _merge_stats(gstat, groups):
    """(n, mean, var) per group of consecutive units from the per-wave partials {count, shift, sum (y - shift),
    sum (y - shift)^2}, merged about the first unit's shift in fp64 (as gn_merge_stats does on the device)."""
    st = gstat.double().reshape(groups, -1, 4)
    cnt, d, s1, s2 = st[..., 0], st[..., 1] - st[:, :1, 1], st[..., 2], st[..., 3]
    n = cnt.sum(1)
    m1 = (s1 + cnt * d).sum(1) / n
    var = ((s2 + 2.0 * d * s1 + cnt * d * d).sum(1) / n - m1 * m1).clamp_min(0.0)
    return n, st[:, 0, 1] + m1, var


def _dwm_fwd(shape, K, form, units, seed=0, offset=0.0):
    """One guarded MFMA forward; returns (x, y, gstat) (gstat None unless form == 'gs')."""
    B, C, H, W = shape
    pad = (K - 1) // 2
    tag = f"mfma {form} {shape} K{K}"
    g = _gen(3000 * K + H + W + seed)
    x = _randn(g, B, C, H, W).to(BF16)
    w = (_randn(g, C, K, K) * 0.2).to(BF16).float()           # taps the kernel's bf16 rounding leaves as they are
    fwd = form in ("plain", "gs")
    b = _randn(g, C) * 0.1 + offset if fwd else None
    nz = _randn(g, H, W) if fwd else None
    rs = _randn(g, B, C, H, W).to(BF16) if form == "flip_res" else None
    plane = _randn(g, H, W) if form == "flip_nplane" else None
    assert _lib.vfm_dwconv2d_fwd_mfma_units(B, C, H, W, K, pad) == units
    c = Case()
    xv, wv, bv, nv, rv, pv = (c.inp(n, t) for n, t in (("x", x), ("w", w), ("bias", b), ("noise", nz), ("res", rs),
                                                       ("nplane", plane)))
    y = c.out("y", shape, BF16)
    npart = c.out("npart", (units,)) if plane is not None else None
    gstat = c.out("gstat", (units, 4)) if form == "gs" else None
    if form == "gs":
        rc = _lib.vfm_dwconv2d_fwd_mfma_gs(_p(xv), _p(wv), _p(bv), _p(nv), _p(y), _p(gstat), B, C, H, W, K, pad, _st())
    else:
        rc = _lib.vfm_dwconv2d_fwd_mfma_nz(_p(xv), _p(wv), _p(bv), _p(nv), _p(rv), _p(y), _p(pv), _p(npart), B, C, H,
                                           W, K, pad, int(not fwd), _st())
    assert rc == 0 and rc != NO_KERNEL, rc
    c.check()
    _check(tag, y, R.dwconv(x, w, b, nz, rs, pad, not fwd), (1 if fwd else 4) * 1.5e-2)
    if npart is not None:
        prod = x.double() * plane.double()
        got, exact, bound = float(npart.double().sum()), float(prod.sum()), 1e-5 * float(prod.abs().sum())
        print(f"{tag}: npart sum {got:.6e} exact {exact:.6e} (bound {bound:.2e})")
        assert abs(got - exact) <= bound
    if gstat is not None:
        n, mean, var = _merge_stats(gstat, B * C)
        yd = y.double().reshape(B * C, -1)
        mref, vref = yd.mean(1), yd.var(1, unbiased=False)
        assert bool((n == H * W).all()), n
        em = float((mean - mref).abs().max() / (mref.abs() + vref.sqrt()).max())
        ev = float((var - vref).abs().max() / vref.max())
        print(f"{tag}: merged mean err {em:.3e}, var err {ev:.3e} (tol 2e-5)")
        assert em < 2e-5 and ev < 2e-5, (em, ev)
    return x, y, gstat


@pytest.mark.parametrize("form", ["plain", "flip_res", "flip_nplane", "gs"])
@pytest.mark.parametrize("row,K", _shape_k(DWM_FWD), ids=_id)
def test_dwconv_mfma_fwd(row, K, form):
    shape, units = row
    _dwm_fwd(shape, K, form, units)


@pytest.mark.parametrize("row,K", _shape_k(DWM_WGRAD), ids=_id)
def test_dwconv_mfma_wgrad(row, K):
    """per > 1 bands per wave (the band loop and its double buffering) with a last wave of fewer bands; the tiles
    value pins the plan branch."""
    shape, tiles = row
    B, C, H, W = shape
    pad = (K - 1) // 2
    assert _lib.vfm_dwconv2d_bwd_weight_mfma_tiles(B, C, H, W, K, pad) == tiles
    g = _gen(4000 * K + H + W)
    x, dy = _randn(g, B, C, H, W).to(BF16), _randn(g, B, C, H, W).to(BF16)
    c = Case()
    xv, dv = c.inp("x", x), c.inp("dy", dy)
    part = c.out("partial", (tiles, C, K * K + 1))
    rc = _lib.vfm_dwconv2d_bwd_weight_mfma(_p(xv), _p(dv), _p(part), B, C, H, W, K, pad, _st())
    assert rc == 0 and rc != NO_KERNEL, rc
    c.check()
    _reduce_and_check(c, part, x, dy, K, pad, 1e-5, None, f"mfma wgrad {shape} K{K}")


# ------------------------------------------------------------------------------------------------------------------
# GroupNorm: vfm_group_norm_fwd_pc, vfm_group_norm_bwd + vfm_colsum2_f32, vfm_group_norm_fwd_stats

def _gn_params(g, B, C, with_style):
    w, b = 1 + 0.1 * _randn(g, C), 0.1 * _randn(g, C)
    return w, b, (1 + 0.3 * _randn(g, B, C)) if with_style else None


@pytest.mark.parametrize("with_style", [False, True], ids=["plain", "style"])
@pytest.mark.parametrize("dt_in,dt_out", GN_PAIRS, ids=_id)
@pytest.mark.parametrize("shape", GN_SHAPES, ids=_id)
def test_group_norm(shape, dt_in, dt_out, with_style):
    B, C, H, W, G = shape
    HW = H * W
    g = _gen(sum(shape))
    x = (_randn(g, B, C, H, W) * 3 + 1.5).to(dt_in)
    w, b, s = _gn_params(g, B, C, with_style)
    worst = dt_out if dt_out != F32 else dt_in
    tag = f"group_norm {shape} {_id(dt_in)}->{_id(dt_out)} style={with_style}"
    yref, mref, rref = R.group_norm_fwd(x, G, w, b, s)
    for pieces in ([False, True] if dt_out == F32 and HW % 8 == 0 else [False]):
        c = Case()
        xv, wv, bv, sv = (c.inp(n, t) for n, t in (("x", x), ("w", w), ("b", b), ("s", s)))
        y, mean, rstd = c.out("y", x.shape, dt_out), c.out("mean", (B * G,)), c.out("rstd", (B * G,))
        yp = c.out("y_pieces", (3, x.numel()), BF16) if pieces else None
        rc = _lib.vfm_group_norm_fwd_pc(_p(xv), _p(wv), _p(bv), _p(sv), _p(y), _p(yp), _p(mean), _p(rstd),
                                        _code(dt_in), _code(dt_out), B, C, G, HW, 1e-5, _st())
        assert rc == 0, rc
        c.check()
        _check(f"{tag} pieces={pieces} y", y, yref, _tol(worst))
        _check_stats(tag, mean, rstd, mref, rref)
        if pieces:
            assert torch.equal(yp.view(torch.int16), R.split3(y).view(torch.int16)), "pieces differ from the split"
    # backward on the kernel's own statistics, then the column sums of its per-sample parts
    dy = _randn(g, B, C, H, W).to(dt_out)
    c = Case()
    xv, dv, mv, rv, wv, bv, sv = (c.inp(n, t) for n, t in (("x", x), ("dy", dy), ("mean", mean), ("rstd", rstd),
                                                           ("w", w), ("b", b), ("s", s)))
    dx, dwp, dbp = c.out("dx", x.shape, dt_in), c.out("dw_part", (B, C)), c.out("db_part", (B, C))
    ds = c.out("ds", (B, C)) if with_style else None
    rc = _lib.vfm_group_norm_bwd(_p(xv), _p(dv), _p(mv), _p(rv), _p(wv), _p(bv), _p(sv), _p(dx), _p(dwp), _p(dbp),
                                 _p(ds), _code(dt_in), _code(dt_out), B, C, G, HW, _st())
    assert rc == 0, rc
    c.check()
    dxr, dwr, dbr, dsr = R.group_norm_bwd(x, dy, G, w, b, s)
    _check(tag + " dx", dx, dxr, 4 * _tol(worst))
    _check(tag + " dw_part", dwp, dwr, 4 * _tol(worst))
    _check(tag + " db_part", dbp, dbr, 4 * _tol(worst))
    if ds is not None:
        _check(tag + " ds", ds, dsr, 4 * _tol(worst))
    _colsum2(dwp, dbp, None, tag, null=None)


def _colsum2(a, b, scale, tag, null):
    rows, cols = a.shape
    c = Case()
    av, bv, sv = c.inp("a", a), c.inp("b", b), c.inp("scale_a", scale)
    oa = None if null == "out_a" else c.out("out_a", (cols,))
    ob = None if null == "out_b" else c.out("out_b", (cols,))
    rc = _lib.vfm_colsum2_f32(_p(av), _p(bv), _p(sv), _p(oa), _p(ob), rows, cols, _st())
    assert rc == 0, rc
    c.check()
    if oa is not None:
        _check(tag + " colsum a", oa, a.double().sum(0) * (1.0 if scale is None else scale.double()), 2e-5)
    if ob is not None:
        _check(tag + " colsum b", ob, b.double().sum(0), 2e-5)


@pytest.mark.parametrize("null", ["out_a", "out_b", None])
def test_colsum2_null_output_and_scale(null):
    """17 and 40 rows: one partial and three rounds of the 16-row batches; 300 columns: a partial second block."""
    g = _gen(17)
    for rows in (17, 40):
        _colsum2(_randn(g, rows, 300), _randn(g, rows, 300), 1 + 0.2 * _randn(g, 300), f"colsum2 {rows}x300", null)


@pytest.mark.parametrize("dt_out", [BF16, F32], ids=_id)
@pytest.mark.parametrize("row", GN_STATS, ids=_id)
def test_group_norm_from_dwconv_stats(row, dt_out):
    """vfm_dwconv2d_fwd_mfma_gs (guarded, with a common offset of 40 on the bias: the shifted partial sums) feeding
    vfm_group_norm_fwd_stats: a GroupNorm of the stored bf16 conv output against the fp64 GroupNorm of the same
    values."""
    (B, C, H, W, G), units = row
    K = 7
    _, d, gstat = _dwm_fwd((B, C, H, W), K, "gs", units, offset=40.0)
    g = _gen(sum(row[0]))
    w, b, s = _gn_params(g, B, C, True)
    c = Case()
    xv, wv, bv, sv, tv = (c.inp(n, t) for n, t in (("x", d), ("w", w), ("b", b), ("s", s), ("stats", gstat)))
    y, mean, rstd = c.out("y", d.shape, dt_out), c.out("mean", (B * G,)), c.out("rstd", (B * G,))
    rc = _lib.vfm_group_norm_fwd_stats(_p(xv), _p(wv), _p(bv), _p(sv), _p(y), _p(mean), _p(rstd), _p(tv),
                                       units // (B * C), _code(BF16), _code(dt_out), B, C, G, H * W, 1e-5, _st())
    assert rc == 0, rc
    c.check()
    yref, mref, rref = R.group_norm_fwd(d, G, w, b, s)
    tag = f"group_norm stats {row[0]} ->{_id(dt_out)}"
    _check(tag + " y", y, yref, _tol(dt_out))
    _check_stats(tag, mean, rstd, mref, rref)


@pytest.mark.parametrize("dt_in,dt_out", [(i, o) for i in (F32, F16, BF16) for o in (F32, F16, BF16)
                                          if (i, o) not in ((BF16, BF16), (BF16, F32))], ids=_id)
@pytest.mark.parametrize("row", GN_STATS[1:], ids=_id)
def test_group_norm_stats_declines_other_dtypes(row, dt_in, dt_out):
    (B, C, H, W, G), units = row
    g = _gen(3)
    c = Case()
    xv = c.inp("x", _randn(g, B, C, H, W).to(dt_in))
    tv = c.inp("stats", torch.ones(units, 4, device=DEV))
    y, mean, rstd = c.out("y", (B, C, H, W), dt_out), c.out("mean", (B * G,)), c.out("rstd", (B * G,))
    rc = _lib.vfm_group_norm_fwd_stats(_p(xv), None, None, None, _p(y), _p(mean), _p(rstd), _p(tv), units // (B * C),
                                       _code(dt_in), _code(dt_out), B, C, G, H * W, 1e-5, _st())
    assert rc == NO_KERNEL, rc
    c.check(written=False)


# ------------------------------------------------------------------------------------------------------------------
# Row kernels: vfm_scale_bias_gelu_fwd/_bwd (_pc), vfm_layer_scale_residual_fwd/_bwd (_bwd_pc)

def _gelu(shape, dt, *, with_scale=True, want_scale_rows=True, pieces=False, P_call=None, expect=0):
    B, O, P = shape
    Pc = P if P_call is None else P_call
    g = _gen(B * O + P)
    h = (_randn(g, B, O, P) * 2).to(dt)
    s = torch.rand(B, O, generator=g, device=DEV) + 0.5 if with_scale else None
    b = _randn(g, O) * 0.3
    dg = _randn(g, B, O, P).to(dt)
    tag = f"gelu {shape} {_id(dt)} scale={with_scale} pieces={pieces}"
    c = Case()
    hv, sv, bv = c.inp("h", h), c.inp("scale", s), c.inp("bias", b)
    out = c.out("g", shape, dt)
    gp = c.out("g_pieces", (3, h.numel()), BF16) if pieces else None
    if pieces:
        rc = _lib.vfm_scale_bias_gelu_fwd_pc(_p(hv), _p(sv), _p(bv), _p(out), _p(gp), _code(dt), B, O, Pc, _st())
    else:
        rc = _lib.vfm_scale_bias_gelu_fwd(_p(hv), _p(sv), _p(bv), _p(out), _code(dt), B, O, Pc, _st())
    assert rc == expect, rc
    c.check(written=expect == 0)
    if expect == 0:
        _check(tag + " g", out, R.gelu_fwd(h, s, b), _tol(dt))
        if pieces:
            assert torch.equal(gp.view(torch.int16), R.split3(out).view(torch.int16)), "pieces differ from the split"
    c = Case()
    hv, dv, sv, bv = c.inp("h", h), c.inp("dg", dg), c.inp("scale", s), c.inp("bias", b)
    dh = c.out("dh", shape, dt)
    dhp = c.out("dh_pieces", (3, h.numel()), BF16) if pieces else None
    r0 = c.out("d_scale_rows", (B * O,)) if want_scale_rows else None
    r1 = c.out("d_bias_rows", (B * O,))
    if pieces:
        rc = _lib.vfm_scale_bias_gelu_bwd_pc(_p(hv), _p(dv), _p(sv), _p(bv), _p(dh), _p(dhp), _p(r0), _p(r1),
                                             _code(dt), B, O, Pc, _st())
    else:
        rc = _lib.vfm_scale_bias_gelu_bwd(_p(hv), _p(dv), _p(sv), _p(bv), _p(dh), _p(r0), _p(r1), _code(dt), B, O,
                                          Pc, _st())
    assert rc == expect, rc
    c.check(written=expect == 0)
    if expect == 0:
        dhr, r0r, r1r = R.gelu_bwd(h, dg, s, b)
        _check(tag + " dh", dh, dhr, 4 * _tol(dt))
        if r0 is not None:
            _check(tag + " d_scale_rows", r0, r0r.reshape(-1), 4 * _tol(dt))
        _check(tag + " d_bias_rows", r1, r1r.reshape(-1), 4 * _tol(dt))
        if pieces:
            assert torch.equal(dhp.view(torch.int16), R.split3(dh).view(torch.int16)), "pieces differ from the split"


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=_id)
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=_id)
def test_scale_bias_gelu(shape, dt):
    _gelu(shape, dt)
    if dt == F32:
        _gelu(shape, dt, pieces=True)


@pytest.mark.parametrize("form", ["no_scale", "no_scale_rows"])
def test_scale_bias_gelu_null_scale_and_rows(form):
    _gelu((3, 5, 520), F32, with_scale=form != "no_scale", want_scale_rows=False)


def _lsr(shape, dt_y, dt_x, *, pieces=False, P_call=None, expect=0):
    B, C, P = shape
    Pc = P if P_call is None else P_call
    g = _gen(B * C + P + 1)
    y, x = _randn(g, B, C, P).to(dt_y), _randn(g, B, C, P).to(dt_x)
    b, gm = 0.1 * _randn(g, C), 0.5 + 0.2 * _randn(g, C)
    dout = _randn(g, B, C, P).to(dt_x)
    worst = dt_y if dt_y != F32 else dt_x
    tag = f"layer_scale_residual {shape} {_id(dt_y)}/{_id(dt_x)} pieces={pieces}"
    c = Case()
    yv, bv, gv, xv = c.inp("y", y), c.inp("bias", b), c.inp("gamma", gm), c.inp("x_in", x)
    out = c.out("out", shape, dt_x)
    rc = _lib.vfm_layer_scale_residual_fwd(_p(yv), _p(bv), _p(gv), _p(xv), _p(out), _code(dt_y), _code(dt_x), B, C,
                                           Pc, _st())
    assert rc == expect, rc
    c.check(written=expect == 0)
    if expect == 0:
        _check(tag + " out", out, R.lsr_fwd(y, b, gm, x), _tol(worst))
    c = Case()
    yv, bv, gv, dv = c.inp("y", y), c.inp("bias", b), c.inp("gamma", gm), c.inp("dout", dout)
    dy = c.out("dy", shape, dt_y)
    dyp = c.out("dy_pieces", (3, y.numel()), BF16) if pieces else None
    r0, r1 = c.out("d_gamma_rows", (B * C,)), c.out("d_sum_rows", (B * C,))
    if pieces:
        rc = _lib.vfm_layer_scale_residual_bwd_pc(_p(yv), _p(bv), _p(gv), _p(dv), _p(dy), _p(dyp), _p(r0), _p(r1),
                                                  _code(dt_y), _code(dt_x), B, C, Pc, _st())
    else:
        rc = _lib.vfm_layer_scale_residual_bwd(_p(yv), _p(bv), _p(gv), _p(dv), _p(dy), _p(r0), _p(r1), _code(dt_y),
                                               _code(dt_x), B, C, Pc, _st())
    assert rc == expect, rc
    c.check(written=expect == 0)
    if expect == 0:
        dyr, r0r, r1r = R.lsr_bwd(y, b, gm, dout)
        _check(tag + " dy", dy, dyr, 4 * _tol(worst))
        _check(tag + " d_gamma_rows", r0, r0r.reshape(-1), 4 * _tol(worst))
        _check(tag + " d_sum_rows", r1, r1r.reshape(-1), 4 * _tol(worst))
        if pieces:
            assert torch.equal(dyp.view(torch.int16), R.split3(dy).view(torch.int16)), "pieces differ from the split"


@pytest.mark.parametrize("dt_y,dt_x", LSR_PAIRS, ids=_id)
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=_id)
def test_layer_scale_residual(shape, dt_y, dt_x):
    _lsr(shape, dt_y, dt_x)
    if dt_y == F32:
        _lsr(shape, dt_y, dt_x, pieces=True)


@pytest.mark.parametrize("dt", [F32, BF16], ids=_id)
def test_row_kernels_reject_a_row_length_off_the_vector_width(dt):
    """P % 8 != 0: VFM_ERR_ARGS from all four entries, nothing written."""
    _gelu((2, 3, 16), dt, P_call=12, expect=ERR_ARGS)
    _lsr((2, 3, 16), dt, dt, P_call=12, expect=ERR_ARGS)


# ------------------------------------------------------------------------------------------------------------------
# PixelShuffle + replicate pad + blur and its adjoint

def _taps(taps):
    s = float(sum(taps))
    return (ctypes.c_float * 8)(*([t / s for t in taps] + [0.0] * (8 - len(taps)))), len(taps)


@pytest.mark.parametrize("dt", [F32, BF16], ids=_id)
@pytest.mark.parametrize("taps", BLUR_TAPS, ids=_id)
@pytest.mark.parametrize("shape,r", BLUR_SHAPES, ids=_id)
def test_shuffle_blur(shape, r, taps, dt):
    B, Cr, H, W = shape
    C = Cr // (r * r)
    g = _gen(sum(shape) + len(taps))
    x, dout = _randn(g, *shape).to(dt), _randn(g, B, C, H * r, W * r).to(dt)
    tp, K = _taps(taps)
    tag = f"shuffle_blur {shape} r{r} K{K} {_id(dt)}"
    c = Case()
    xv = c.inp("x", x)
    y = c.out("y", (B, C, H * r, W * r), dt)
    rc = _lib.vfm_shuffle_blur_fwd(_p(xv), _p(y), tp, K, _code(dt), B, C, H, W, r, _st())
    assert rc == 0, rc
    c.check()
    _check(tag + " fwd", y, R.shuffle_blur_fwd(x, taps, r), _tol(dt))
    c = Case()
    dv = c.inp("dout", dout)
    dx = c.out("dx", shape, dt)
    rc = _lib.vfm_shuffle_blur_bwd(_p(dv), _p(dx), tp, K, _code(dt), B, C, H, W, r, _st())
    assert rc == 0, rc
    c.check()
    _check(tag + " bwd", dx, R.shuffle_blur_bwd(dout, taps, r), 4 * _tol(dt))


# ------------------------------------------------------------------------------------------------------------------
# Channel RMS norm

def _rms(shape, rows, null=None):
    B, C, P = shape
    scale = float(C) ** 0.5
    g = _gen(B + C + P)
    x, dy = _randn(g, B, C, P), _randn(g, B, C, P)
    x[B - 1, :, 1] = 0.0                                   # one all-zero column: the clamped norm
    gamma = 1 + 0.2 * _randn(g, C)
    tag = f"channel_rms_norm {shape}" + (f" without {null}" if null else "")
    live = torch.ones(B, P, dtype=torch.bool, device=DEV)
    live[B - 1, 1] = False
    c = Case()
    xv, gv = c.inp("x", x), c.inp("gamma", gamma)
    y = c.out("y", shape)
    rinv = None if null == "rinv" else c.out("rinv", (B, P))
    rc = _lib.vfm_channel_rms_norm_fwd(_p(xv), _p(gv), _p(y), _p(rinv), B, C, P, scale, _st())
    assert rc == 0, rc
    c.check()
    yr, rinv_ref = R.rms_fwd(x, gamma, scale)
    _check(tag + " y", y, yr, 2e-5)
    if rinv is None:
        return
    _check(tag + " rinv", rinv[live], rinv_ref[live], 2e-5)
    _check(tag + " rinv (clamped)", rinv[~live], rinv_ref[~live], 2e-5)
    assert _lib.vfm_channel_rms_norm_rows(B, C, P) == rows
    c = Case()
    xv, gv, rv, dv = c.inp("x", x), c.inp("gamma", gamma), c.inp("rinv", rinv), c.inp("dy", dy)
    dx = c.out("dx", shape)
    gpart = dgamma = None
    if null != "gpart":
        gpart, dgamma = c.out("gpart", (rows * C,)), c.out("dgamma", (C,))
    rc = _lib.vfm_channel_rms_norm_bwd(_p(xv), _p(gv), _p(rv), _p(dv), _p(dx), _p(gpart), _p(dgamma), B, C, P, scale,
                                       _st())
    assert rc == 0, rc
    c.check()
    dxr, dgr = R.rms_bwd(x, gamma, dy, scale)
    cols = live[:, None, :].expand(B, C, P)
    _check(tag + " dx", dx[cols], dxr[cols], 1e-4)
    _check(tag + " dx (clamped column)", dx[~cols], dxr[~cols], 1e-4)
    if dgamma is not None:
        _check(tag + " dgamma", dgamma, dgr, 1e-4)


@pytest.mark.parametrize("shape,rows", RMS_SHAPES, ids=_id)
def test_channel_rms_norm(shape, rows):
    _rms(shape, rows)


@pytest.mark.parametrize("null", ["rinv", "gpart"])
def test_channel_rms_norm_null_outputs(null):
    _rms(*RMS_SHAPES[0], null=null)


# ------------------------------------------------------------------------------------------------------------------
# ToRGB

@pytest.mark.parametrize("dt", [F32, BF16], ids=_id)
@pytest.mark.parametrize("shape,splits", TORGB_SHAPES, ids=_id)
def test_torgb(shape, splits, dt):
    B, C, P, O = shape
    g = _gen(sum(shape))
    x = _randn(g, B, C, P).to(dt)
    wm = 0.1 * _randn(g, B, O, C) * (1 + 0.3 * _randn(g, B, 1, C))
    bias, dy = _randn(g, O), _randn(g, B, O, P)
    tag = f"torgb {shape} {_id(dt)}"
    c = Case()
    xv, wv, bv = c.inp("x", x), c.inp("wm", wm), c.inp("bias", bias)
    y = c.out("y", (B, O, P))
    rc = _lib.vfm_torgb_fwd(_p(xv), _p(wv), _p(bv), _p(y), _code(dt), B, O, C, P, _st())
    assert rc == 0 and rc != NO_KERNEL, rc
    c.check()
    _check(tag + " y", y, R.torgb_fwd(x, wm, bias), _tol(dt))
    S = _lib.vfm_torgb_bwd_splits(B, C, P)
    assert S == splits
    c = Case()
    xv, dv, wv = c.inp("x", x), c.inp("dy", dy), c.inp("wm", wm)
    dx, tpart = c.out("dx", (B, C, P), dt), c.out("tpart", (B, S, O, C))
    rc = _lib.vfm_torgb_bwd(_p(xv), _p(dv), _p(wv), _p(dx), _p(tpart), _code(dt), B, O, C, P, S, _st())
    assert rc == 0 and rc != NO_KERNEL, rc
    c.check()
    dxr, Tr = R.torgb_bwd(x, dy, wm)
    _check(tag + " dx", dx, dxr, 4 * _tol(dt))
    _check(tag + " T", tpart.double().sum(1), Tr, 4 * _tol(dt))


# ------------------------------------------------------------------------------------------------------------------
# Posterior sample + KL

def _posterior(shape, null=None):
    B, C, P = shape
    g = _gen(B * C + P)
    params = _randn(g, B, 2 * C, P)
    params[:, C:, 0] = 25.0                  # clamped above
    params[:, C:, 1] = -35.0                 # clamped below
    eps, dz, dkl = _randn(g, B, C, P), _randn(g, B, C, P), _randn(g, B)
    tag = f"posterior {shape}" + (f" without {null}" if null else "")
    c = Case()
    pv, ev = c.inp("params", params), c.inp("eps", eps)
    z = None if null == "z" else c.out("z", (B, C, P))
    kl = None if null == "kl" else c.out("kl", (B,))
    rc = _lib.vfm_posterior_fwd(_p(pv), _p(ev), _p(z), _p(kl), B, C, P, _st())
    assert rc == 0, rc
    c.check()
    zr, klr = R.posterior_fwd(params, eps)
    if z is not None:
        _check(tag + " z", z, zr, 1e-6)
    if kl is not None:
        _check(tag + " kl", kl, klr, 1e-6)
    c = Case()
    pv, ev = c.inp("params", params), c.inp("eps", eps)
    zv = None if null == "dz" else c.inp("dz", dz)
    kv = None if null == "dkl" else c.inp("dkl", dkl)
    dp = c.out("dparams", (B, 2 * C, P))
    rc = _lib.vfm_posterior_bwd(_p(pv), _p(ev), _p(zv), _p(kv), _p(dp), B, C, P, _st())
    assert rc == 0, rc
    c.check()
    _check(tag + " dparams", dp, R.posterior_bwd(params, eps, None if zv is None else dz, None if kv is None else dkl),
           1e-5)
    assert float(dp[:, C:, :2].abs().max()) == 0.0          # no gradient beyond either clamp


@pytest.mark.parametrize("shape", POSTERIOR_SHAPES, ids=_id)
def test_posterior(shape):
    _posterior(shape)


@pytest.mark.parametrize("null", ["z", "kl", "dz", "dkl"])
def test_posterior_null_operands(null):
    _posterior(POSTERIOR_SHAPES[0], null=null)


# ------------------------------------------------------------------------------------------------------------------
# The harness itself on the device (both stay inside the 64 KiB pad)

def test_guard_sees_a_row_eight_elements_too_long():
    """vfm_scale_bias_gelu_fwd with P declared 8 larger than the output view's single row: the row's tail lands in the
    sentinel and is reported, element for element."""
    P = 64
    g = _gen(1)
    h = _randn(g, 1, 1, P + 8)
    out, obuf = gb.embed(torch.full((1, 1, P), gb.POISON, device=DEV), fill=gb.SENTINEL)
    assert _lib.vfm_scale_bias_gelu_fwd(_p(h), None, None, _p(out), _code(F32), 1, 1, P + 8, _st()) == 0
    torch.cuda.synchronize()
    assert not gb.intact(out, obuf, gb.SENTINEL)
    hit = gb.touched(out, obuf, gb.SENTINEL)
    base = out.storage_offset()
    assert hit.tolist() == list(range(base + P, base + P + 8)), gb.describe(out, obuf, gb.SENTINEL)
    assert not torch.isnan(out).any()


def test_guard_sees_a_read_one_row_below_the_plane():
    """vfm_dwconv2d_fwd_res on a one-plane input with H declared one row taller than the embedded view: the rows whose
    taps reach the extra row read the poison and say so, where the allocator's finite leftovers would have
    passed a max-error bound."""
    H, W, K = 6, 9, 3
    g = _gen(2)
    x, xbuf = gb.embed(_randn(g, 1, 1, H, W), fill=gb.POISON)
    w = _randn(g, 1, K, K)
    y = torch.full((1, 1, H + 1, W), gb.POISON, device=DEV)
    assert _lib.vfm_dwconv2d_fwd_res(_p(x), _p(w), None, None, None, _p(y), _code(F32), 1, 1, H + 1, W, K, 1, 0,
                                     _st()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[0, 0, H - 1:]).all()) and not torch.isnan(y[0, 0, :H - 1]).any()
    assert gb.intact(x, xbuf, gb.POISON)
    y2 = torch.full((1, 1, H, W), gb.POISON, device=DEV)
    assert _lib.vfm_dwconv2d_fwd_res(_p(x), _p(w), None, None, None, _p(y2), _code(F32), 1, 1, H, W, K, 1, 0,
                                     _st()) == 0
    assert not torch.isnan(y2).any()
