"""Guard bands around the GEMM kernels (csrc/gemm.hip, gemm8.hip, gemm9.hip, sgemm.hip) through
`gemm_hip.try_gemm(..., out=view, route=...)` and `gemm_hip.sgemm(...)`: no stray reads or writes.

Every case runs one product whose operands are views embedded in NaN (tests/guard_bands.py: base 16-B but
not 512-B aligned, optionally pitched rows `ld = extent + 8` and a gap between batch planes), whose output is
a view with `ldc = N + 8` (batched: `sC = M * ldc + 64`) embedded in a finite sentinel and pre-filled with NaN
(beta == 0) and whose scratch (split-K / batch-reduce partials, bf16 piece buffers of fp32 operands) is
substituted by embedded buffers of exactly the size the wrapper asked for. It asserts that
  * the timer region names the intended kernel instantiation (and no other GEMM ran);
  * the result matches the fp64 product within the tolerance of the file that already tests that kernel
    (test_gemm_gpu.py: F32_TOL for f32x6, 1e-5 for bf16 -> fp32, 8e-3 for bf16 out; 1e-6 for sgemm);
  * the result holds no NaN: every element was written, and nothing read from the poison reached it;
  * the fill around the output, around both operands, the bias and every scratch buffer is untouched.
A layout a kernel declines is pinned as declined (None / another region), never skipped."""
import pytest
import torch

import guard_bands as gb
from torch_utils import custom_ops
from torch_utils.ops import gemm_hip, kernel_timer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_TOL = 2e-6              # tests/test_gemm_gpu.py
BF16_F32_TOL = 1e-5         # bf16 operands, fp32 output (tests/test_gemm_gpu.py)
BF16_OUT_TOL = 8e-3         # one bf16 output rounding (tests/test_gemm_gpu.py, tests/test_gemm9_gpu.py)
SGEMM_TOL = 1e-6            # tests/test_gemm_gpu.py::test_gemm_unsupported_shape_routes_exact_fp32
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
BF16, F32 = torch.bfloat16, torch.float32


def _tb(v):
    return "true" if v else "false"


def _vals(shape, dtype, g):
    return (torch.rand(*shape, generator=g) * 2 - 1).to(dtype).to(DEV)


def _embed_operand(t, contiguous_last, pitched):
    """t [z, rows, cols] embedded in NaN with its last (contiguous_last) or middle dim contiguous; pitched:
    rows of extent + 8 elements and 64 more between the planes."""
    order = (0, 1, 2) if contiguous_last else (0, 2, 1)
    inner = t.shape[2] if contiguous_last else t.shape[1]
    return gb.embed(t, fill=gb.POISON, order=order, pitch=inner + 8 if pitched else None,
                    gap=64 if pitched and t.shape[0] > 1 else 0)


class Scratch:
    """Stands in for gemm_hip._workspace / gemm_hip._alloc: every buffer embedded, of exactly the size asked for.
    fp32 partials: NaN inside (a partial that is read before it is written shows in the result), the sentinel
    around; bf16 piece buffers are an output of vfm_split_f32 and an input of the product: NaN inside and around."""

    def __init__(self):
        self.items = []

    def _new(self, shape, dtype, dev):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        fill = gb.SENTINEL if dtype == torch.float32 else gb.POISON
        v, buf = gb.embed(torch.full(shape, gb.POISON, dtype=dtype, device=dev), fill=fill)
        self.items.append((v, buf, fill))
        return v

    def workspace(self, n, dev):
        return self._new(n, torch.float32, dev)

    def alloc(self, shape, dtype, dev):
        return self._new(shape, dtype, dev)

    def check(self, pieces_written=True):
        for v, buf, fill in self.items:
            assert gb.intact(v, buf, fill), f"scratch {tuple(v.shape)} {v.dtype}: " + gb.describe(v, buf, fill)
            if v.dtype == torch.bfloat16 and pieces_written:
                assert not torch.isnan(v).any(), "piece buffer not written whole"


@pytest.fixture
def scratch(monkeypatch):
    s = Scratch()
    monkeypatch.setattr(gemm_hip, "_workspace", s.workspace)
    monkeypatch.setattr(gemm_hip, "_alloc", s.alloc)
    return s


def _act64(c, act):
    if act == "gelu_tanh":
        return torch.nn.functional.gelu(c, approximate="tanh")
    if act == "gelu":
        return torch.nn.functional.gelu(c)
    return c


def _run(scratch, dtype, M, N, K, *, z=1, shared=None, a_kc=True, b_kc=False, pitched=False, whole=False,
         out_dtype=torch.float32, call="try_gemm", expect=None, tol=None, bias_dim=None, act=None, alpha=1.0,
         beta=0.0, reduce_batch=False, dense_out=False, declined=False, n_scratch=None, seed=0, **kw):
    """One guarded product; `expect`: the one timer region (prefix) that must have run; `declined`: the entry must
    return None and leave everything untouched. whole: the operands are whole tensors (planar pieces) instead of
    embedded views. dense_out: ldc == N, sC == M * N (still embedded)."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + z + seed)
    za, zb = (1 if shared == "A" else z), (1 if shared == "B" else z)
    A = _vals((za, M, K), dtype, g)
    B = _vals((zb, K, N), dtype, g)
    if whole:
        a = A if a_kc else A.transpose(1, 2).contiguous().transpose(1, 2)
        b = B.transpose(1, 2).contiguous().transpose(1, 2) if b_kc else B
        guards = []
    else:
        a, abuf = _embed_operand(A, a_kc, pitched)
        b, bbuf = _embed_operand(B, not b_kc, pitched)
        guards = [("A", a, abuf, gb.POISON), ("B", b, bbuf, gb.POISON)]
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    batched = z > 1
    av = a if (batched and shared != "A") else a[0]
    bv = b if (batched and shared != "B") else b[0]
    oshape = (z, M, N) if batched and not reduce_batch else (M, N)
    C0 = _vals(oshape, out_dtype, g) if beta != 0.0 else torch.full(oshape, gb.POISON, dtype=out_dtype, device=DEV)
    out, obuf = gb.embed(C0, fill=gb.SENTINEL, pitch=None if dense_out else N + 8,
                         gap=0 if dense_out or len(oshape) == 2 else 64)
    guards.append(("out", out, obuf, gb.SENTINEL))
    bias = None
    if bias_dim is not None:
        bias, biasbuf = gb.embed(_vals((M if bias_dim == 0 else N,), torch.float32, g), fill=gb.POISON)
        guards.append(("bias", bias, biasbuf, gb.POISON))
    args = dict(out=out, bias=bias, bias_dim=bias_dim, act=act, alpha=alpha, beta=beta, reduce_batch=reduce_batch)
    kernel_timer.enable(True)
    try:
        if call == "sgemm":
            res = gemm_hip.sgemm(av, bv, **args, **kw)
        else:
            res = gemm_hip.try_gemm(av, bv, out_dtype=out_dtype, **args, **kw)
        names = list(kernel_timer.summary())
    finally:
        kernel_timer.enable(False)
    torch.cuda.synchronize()
    for what, v, buf, fill in guards:
        assert gb.intact(v, buf, fill), f"{what}: " + gb.describe(v, buf, fill)
    if declined:
        assert res is None, f"expected the layout to be declined, ran {names}"
        assert bool(torch.isnan(out).all()), "a declined product wrote its output"
        scratch.check(pieces_written=False)
        return None
    scratch.check()
    if n_scratch is not None:
        assert len(scratch.items) == n_scratch, [tuple(v.shape) for v, _, _ in scratch.items]
    assert res is not None, "no kernel took the product"
    assert res.data_ptr() == out.data_ptr() and res.shape == out.shape
    assert names and all(n.startswith(expect) for n in names), (expect, names)
    ref = alpha * torch.matmul(A.double(), B.double())
    if reduce_batch:
        ref = ref.sum(0)
    elif not batched:
        ref = ref[0]
    if bias is not None:
        ref = ref + (bias.double()[:, None] if bias_dim == 0 else bias.double())
    ref = _act64(ref, act)
    if beta != 0.0:
        ref = ref + beta * C0.double()
    assert not torch.isnan(out).any(), f"{int(torch.isnan(out).sum())} NaN in the result (unwritten or poisoned)"
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"{expect} {M}x{N}x{K}x{z}: rel err {err:.3e} (tol {tol:.1e})")
    assert err < tol, (err, tol)
    return out


@pytest.mark.parametrize("route,dtype", [(("g9", 0), BF16), (("g8", 0), BF16), (("g128", 1), F32)])
def test_guard_sees_a_store_eight_columns_too_wide(route, dtype, monkeypatch):
    """The harness itself on the device: the same product stored through a view eight columns wider than the one
    the guard knows (all of it inside the buffer) is reported, element for element -- what a full-row store past a
    ragged N would look like."""
    monkeypatch.setattr(gemm_hip, "G9", route[0] == "g9")
    M, N, K = 304, 264, 64
    g = torch.Generator().manual_seed(1)
    A, B = _vals((M, K), dtype, g), _vals((K, N + 8), dtype, g)
    out, obuf = gb.embed(torch.full((M, N), gb.POISON, dtype=dtype, device=DEV), fill=gb.SENTINEL, pitch=N + 8)
    wide = obuf.as_strided((M, N + 8), (N + 8, 1), out.storage_offset())
    assert gemm_hip.try_gemm(A, B, out=wide, route=route) is not None
    torch.cuda.synchronize()
    assert not gb.intact(out, obuf, gb.SENTINEL)
    assert gb.touched(out, obuf, gb.SENTINEL).numel() == M * 8
    assert gb.intact(wide, obuf, gb.SENTINEL)


@pytest.mark.parametrize("route,dtype", [(("g9", 0), BF16), (("g8", 0), BF16), (("g128", 1), F32)])
def test_guard_sees_a_read_one_k_tile_too_deep(route, dtype, monkeypatch):
    """And for reads: A claimed one K-tile deeper than the embedded operand (rows pitched K + 72, so every row's extension
    lies in its NaN gap; all of it inside the buffer) against 64 more rows of B that are zero. 0 x poison is NaN:
    every output says so, where the allocator's finite leftovers would have given the exact product."""
    monkeypatch.setattr(gemm_hip, "G9", route[0] == "g9")
    M, N, K = 304, 264, 64
    g = torch.Generator().manual_seed(2)
    a, abuf = gb.embed(_vals((M, K), dtype, g), fill=gb.POISON, pitch=K + 72)
    deep = abuf.as_strided((M, K + 64), (K + 72, 1), a.storage_offset())
    B = torch.cat([_vals((K, N), dtype, g), torch.zeros(64, N, dtype=dtype, device=DEV)])
    out = gemm_hip.try_gemm(deep, B, route=route)
    assert out is not None and bool(torch.isnan(out).all())
    assert not torch.isnan(gemm_hip.try_gemm(a, B[:K], route=route)).any()


def _tag(dtype):
    return "bf16" if dtype == BF16 else "f32x6"


def _tol(dtype, out_dtype=F32):
    return F32_TOL if dtype == F32 else (BF16_F32_TOL if out_dtype == F32 else BF16_OUT_TOL)


# ------------------------------------------------------------------------------------------------------------------
# the 128-tile kernel (csrc/gemm.hip, vfm_gemm): ragged M, N and K tails inside a tile

G128 = (200, 136, 72)


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_g128_layouts(scratch, dtype, a_kc, b_kc, pitched):
    _run(scratch, dtype, *G128, a_kc=a_kc, b_kc=b_kc, pitched=pitched, route=("g128", 1), n_scratch=0,
         expect=f"gemm<{_tag(dtype)},{_tb(a_kc)},{_tb(b_kc)},true>", tol=_tol(dtype))


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("form", ["shared_a", "shared_b", "splits3", "reduce", "reduce_splits3"])
def test_g128_batched_split_reduce(scratch, dtype, a_kc, b_kc, form):
    kw = dict(route=("g128", 3 if form.endswith("splits3") else 1), pitched=True)
    if form in ("shared_a", "shared_b"):
        kw.update(z=3, shared=form[-1].upper(), n_scratch=0)
    elif form != "splits3":
        kw.update(z=3, reduce_batch=True)
    if form in ("splits3", "reduce", "reduce_splits3"):
        kw.update(n_scratch=1)
    _run(scratch, dtype, *G128, a_kc=a_kc, b_kc=b_kc, expect=f"gemm<{_tag(dtype)},{_tb(a_kc)},{_tb(b_kc)},true>",
         tol=_tol(dtype), **kw)
    if "n_scratch" in kw and kw["n_scratch"]:
        z, s = (3, True) if form != "splits3" else (1, False)
        n = gemm_hip._lib.vfm_gemm_workspace_floats(G128[0], G128[1], z, kw["route"][1], int(s))
        assert scratch.items[0][0].numel() == n


@pytest.mark.parametrize("dtype,out_dtype", [(BF16, BF16), (BF16, F32), (F32, F32)])
@pytest.mark.parametrize("bias_dim,act", [(0, "gelu_tanh"), (1, "gelu")])
@pytest.mark.parametrize("splits", [1, 3])
def test_g128_epilogue(scratch, dtype, out_dtype, bias_dim, act, splits):
    _run(scratch, dtype, *G128, a_kc=True, b_kc=True, pitched=True, route=("g128", splits), out_dtype=out_dtype,
         bias_dim=bias_dim, act=act, alpha=0.75, z=2, shared="A",
         expect=f"gemm<{_tag(dtype)},true,true,{_tb(out_dtype == F32)}>", tol=_tol(dtype, out_dtype))


@pytest.mark.parametrize("dtype,out_dtype", [(BF16, BF16), (BF16, F32), (F32, F32)])
def test_g128_beta_accumulates_inside_pitched_out(scratch, dtype, out_dtype):
    _run(scratch, dtype, *G128, a_kc=True, b_kc=False, pitched=True, route=("g128", 1), out_dtype=out_dtype, z=2,
         alpha=0.5, beta=-2.0, expect=f"gemm<{_tag(dtype)},true,false,{_tb(out_dtype == F32)}>",
         tol=_tol(dtype, out_dtype))


# ------------------------------------------------------------------------------------------------------------------
# gemm8 (csrc/gemm8.hip): 256 tiles, LDS-DMA staging through buffer descriptors, LDS-staged 16-B store epilogue

@pytest.fixture(params=[1, 0], ids=["deep", "one_ahead"])
def g8(request, monkeypatch):
    """Both K-tile staging schedules; bf16 and fp32 products kept on gemm8 (not gemm9 / its piece form)."""
    monkeypatch.setattr(gemm_hip, "G9", False)
    monkeypatch.setattr(gemm_hip, "G9_F32", False)
    prev = gemm_hip._lib.vfm_gemm8_set_schedule(request.param)
    yield request.param
    gemm_hip._lib.vfm_gemm8_set_schedule(prev)


def _g8_region(dtype, a_kc, b_kc, out_dtype=F32):
    return f"gemm8<{_tag(dtype)},{_tb(a_kc)},{_tb(b_kc)},{_tb(out_dtype == F32)}>"


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("dtype,out_dtype", [(BF16, BF16), (BF16, F32), (F32, F32)])
def test_g8_layouts(scratch, g8, dtype, out_dtype, a_kc, b_kc, pitched):
    """(520, 264, 128): ragged last tiles in M and N next to full 256 x 256 ones; fp32 operands as views: the
    stacked piece split (vfm_split_f32 along K) into embedded piece buffers."""
    _run(scratch, dtype, 520, 264, 128, a_kc=a_kc, b_kc=b_kc, pitched=pitched, route=("g8", 0), out_dtype=out_dtype,
         n_scratch=2 if dtype == F32 else 0, expect=_g8_region(dtype, a_kc, b_kc, out_dtype), tol=_tol(dtype, out_dtype))


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("form", ["one_tile", "z2", "z2_shared_a", "z2_shared_b", "kchunk2", "kchunk4"])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_g8_tile_batch_split(scratch, g8, dtype, a_kc, b_kc, form):
    """One full tile over one K-tile (the full-row store form alone), batched and batch-shared operands, split-K
    with even and ragged last chunks (K = 384: 6 K-tiles, 36 virtual ones for f32x6)."""
    shape, kw = (520, 264, 128), dict(route=("g8", 0), pitched=True)
    if form == "one_tile":
        shape = (256, 256, 64)
    elif form.startswith("z2"):
        kw.update(z=2, shared=form[-1].upper() if "shared" in form else None)
    else:
        shape = (520, 264, 384)
        kw.update(route=("g8", int(form[-1])))
    _run(scratch, dtype, *shape, a_kc=a_kc, b_kc=b_kc, expect=_g8_region(dtype, a_kc, b_kc), tol=_tol(dtype), **kw)
    if form.startswith("kchunk"):
        prec = custom_ops.VFM_BF16 if dtype == BF16 else custom_ops.f32_precision()[0]
        n = gemm_hip._lib.vfm_gemm8_workspace_floats(prec, *shape, 1, int(form[-1]), 0)
        ws = [v for v, _, _ in scratch.items if v.dtype == F32]
        assert n > 0 and len(ws) == 1 and ws[0].numel() == n


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_g8_batch_reduced(scratch, g8, dtype, a_kc, b_kc, monkeypatch):
    """sum_b dy[b] x[b]^T on gemm8's split-K over the batch-concatenated K (SPLIT8), partials in an embedded
    workspace of exactly vfm_gemm8_workspace_floats."""
    monkeypatch.setattr(gemm_hip, "SPLIT8", True)
    O, I, P, z = 304, 264, 320, 3
    _run(scratch, dtype, O, I, P, z=z, reduce_batch=True, a_kc=a_kc, b_kc=b_kc, pitched=True,
         expect=_g8_region(dtype, a_kc, b_kc), tol=_tol(dtype))
    ws = [v for v, _, _ in scratch.items if v.dtype == F32]
    assert len(ws) == 1 and ws[0].numel() >= O * I


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("form", ["plain", "z2_shared_a", "kchunk4"])
def test_g8_f32_planar_pieces(scratch, g8, a_kc, b_kc, form):
    """fp32 operands that are whole tensors: planar pieces [3][numel] (one vfm_split_f32 over the tensor) in
    embedded piece buffers, read by gemm8 through the piece stride."""
    shape, kw = (520, 264, 128), dict(route=("g8", 0))
    if form == "z2_shared_a":
        kw.update(z=2, shared="A")
    elif form == "kchunk4":
        shape, kw = (520, 264, 384), dict(route=("g8", 4))
    _run(scratch, F32, *shape, a_kc=a_kc, b_kc=b_kc, whole=True, expect=_g8_region(F32, a_kc, b_kc), tol=F32_TOL, **kw)
    pieces = [v for v, _, _ in scratch.items if v.dtype == BF16]
    assert len(pieces) == 2 and all(p.dim() == 2 and p.shape[0] == 3 for p in pieces)      # [3][numel], not stacked


@pytest.mark.parametrize("dtype,out_dtype", [(BF16, BF16), (BF16, F32), (F32, F32)])
@pytest.mark.parametrize("bias_dim,act", [(0, "gelu_tanh"), (1, "gelu")])
def test_g8_epilogue(scratch, g8, dtype, out_dtype, bias_dim, act):
    _run(scratch, dtype, 520, 264, 128, a_kc=True, b_kc=False, pitched=True, route=("g8", 0), out_dtype=out_dtype,
         bias_dim=bias_dim, act=act, alpha=0.75, z=2, shared="A", expect=_g8_region(dtype, True, False, out_dtype),
         tol=_tol(dtype, out_dtype))


@pytest.mark.parametrize("dtype,out_dtype", [(BF16, BF16), (BF16, F32), (F32, F32)])
def test_g8_beta_accumulates_inside_pitched_out(scratch, g8, dtype, out_dtype):
    _run(scratch, dtype, 520, 264, 128, a_kc=True, b_kc=True, pitched=True, route=("g8", 0), out_dtype=out_dtype,
         z=2, alpha=0.5, beta=-2.0, expect=_g8_region(dtype, True, True, out_dtype), tol=_tol(dtype, out_dtype))


# ------------------------------------------------------------------------------------------------------------------
# gemm9 (csrc/gemm9.hip): bf16 products (vfm_gemm9 / vfm_gemm9_ex), persistent and one-workgroup-per-tile forms

@pytest.fixture(params=[1, 0], ids=["persistent", "per_tile"])
def g9mode(request):
    prev = gemm_hip._lib.vfm_gemm9_set_mode(request.param)
    yield request.param
    gemm_hip._lib.vfm_gemm9_set_mode(prev)


def _g9_region(a_kc, b_kc, out_dtype, tag="bf16"):
    return f"gemm9<{tag},{_tb(a_kc)},{_tb(b_kc)},{_tb(out_dtype == F32)}>"


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [(304, 264, 64), (257, 136, 192)])
@pytest.mark.parametrize("out_dtype", [BF16, F32])
def test_g9_layouts(scratch, g9mode, out_dtype, M, N, K, a_kc, b_kc, pitched):
    """An M-contiguous A with M % 8 != 0 (16-B DMA chunks would straddle rows) is declined by every bf16 kernel:
    try_gemm returns None and writes nothing; the K-contiguous storage of the same values (the cases beside it)
    is the route that takes the product."""
    _run(scratch, BF16, M, N, K, a_kc=a_kc, b_kc=b_kc, pitched=pitched, route=("g9", 0), out_dtype=out_dtype,
         n_scratch=0, declined=(M % 8 != 0 and not a_kc), expect=_g9_region(a_kc, b_kc, out_dtype),
         tol=_tol(BF16, out_dtype))


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("shared", ["A", "B", None])
def test_g9_batched(scratch, g9mode, shared, a_kc, b_kc):
    _run(scratch, BF16, 304, 264, 64, z=3, shared=shared, a_kc=a_kc, b_kc=b_kc, pitched=True, route=("g9", 0),
         out_dtype=BF16, expect=_g9_region(a_kc, b_kc, BF16), tol=BF16_OUT_TOL)


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("out_dtype", [BF16, F32])
@pytest.mark.parametrize("form", ["reduce", "split_k"])
def test_g9_reduce_and_split(scratch, g9mode, form, out_dtype, a_kc, b_kc):
    """vfm_gemm9_ex: the batch-reduced weight gradient (O, I, P, z) = (304, 264, 320, 3) through the auto route and
    one split-K product (route "g9r"), partials in an embedded workspace of exactly vfm_gemm9_workspace_floats. The
    one-workgroup-per-tile mode has no split form: it declines (VFM_NO_KERNEL) and gemm8 takes the product."""
    if form == "reduce":
        shape, kw, wsargs = (304, 264, 320), dict(z=3, reduce_batch=True, auto=True), (3, None, 1)
    else:
        shape, kw, wsargs = (304, 264, 512), dict(route=("g9r", 3)), (1, 3, 0)
    region = f"gemm9<bf16,{_tb(a_kc)},{_tb(b_kc)},true>" if g9mode else _g8_region(BF16, a_kc, b_kc, out_dtype)
    _run(scratch, BF16, *shape, a_kc=a_kc, b_kc=b_kc, pitched=True, out_dtype=out_dtype, expect=region,
         tol=_tol(BF16, out_dtype), n_scratch=1 if g9mode else None, **kw)
    if g9mode:
        S = wsargs[1] or gemm_hip._plan(BF16, shape[0], shape[1], shape[2], 3, True, 1, True)[1]
        n = gemm_hip._lib.vfm_gemm9_workspace_floats(*shape, wsargs[0], S, wsargs[2])
        assert n > 0 and scratch.items[0][0].numel() == n


@pytest.mark.parametrize("out_dtype", [BF16, F32])
@pytest.mark.parametrize("bias_dim,act", [(0, "gelu_tanh"), (1, "gelu")])
def test_g9_epilogue(scratch, g9mode, out_dtype, bias_dim, act):
    _run(scratch, BF16, 304, 264, 64, a_kc=True, b_kc=False, pitched=True, route=("g9", 0), out_dtype=out_dtype,
         bias_dim=bias_dim, act=act, alpha=0.75, z=2, shared="A", expect=_g9_region(True, False, out_dtype),
         tol=_tol(BF16, out_dtype))


@pytest.mark.parametrize("out_dtype", [BF16, F32])
def test_g9_beta_accumulates_inside_pitched_out(scratch, g9mode, out_dtype):
    _run(scratch, BF16, 304, 264, 64, a_kc=True, b_kc=True, pitched=True, route=("g9", 0), out_dtype=out_dtype, z=2,
         alpha=0.5, beta=-2.0, expect=_g9_region(True, True, out_dtype), tol=_tol(BF16, out_dtype))


# ------------------------------------------------------------------------------------------------------------------
# f32x6 on gemm9 (vfm_gemm9_pieces) through auto=True with the gemm9 planner

@pytest.fixture
def g9f(monkeypatch):
    monkeypatch.setattr(gemm_hip, "G9F_PLAN", True)
    monkeypatch.setattr(gemm_hip, "G9_F32", True)
    monkeypatch.setattr(gemm_hip, "G9F_BIAS", True)


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("M,N,K,z", [(304, 264, 64, 1), (264, 520, 128, 2)])
def test_g9f_layouts(scratch, g9f, M, N, K, z, a_kc, b_kc, pitched):
    _run(scratch, F32, M, N, K, z=z, a_kc=a_kc, b_kc=b_kc, pitched=pitched, auto=True, n_scratch=2,
         expect=_g9_region(a_kc, b_kc, F32, "f32x6"), tol=F32_TOL)


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("form", ["planar", "shared_a", "bias0", "bias1", "split_k", "reduce"])
def test_g9f_forms(scratch, g9f, form, a_kc, b_kc):
    """Planar pieces of whole tensors, a batch-shared operand, the bias epilogues (alpha != 1), the K split
    (512, 384, 4096) and the batch reduction, each with its partials in an embedded workspace of exactly
    vfm_gemm9_workspace_floats."""
    shape, kw = (304, 264, 64), dict(pitched=True, n_scratch=2)
    if form == "planar":
        kw = dict(whole=True, n_scratch=2)
    elif form == "shared_a":
        shape = (264, 520, 128)
        kw.update(z=2, shared="A")
    elif form.startswith("bias"):
        kw.update(bias_dim=int(form[-1]), alpha=0.75)
    elif form == "split_k":
        shape = (512, 384, 4096)
        kw.update(n_scratch=3)
    else:
        shape = (304, 264, 320)
        kw.update(z=3, reduce_batch=True, n_scratch=3)
    _run(scratch, F32, *shape, a_kc=a_kc, b_kc=b_kc, auto=True, expect=_g9_region(a_kc, b_kc, F32, "f32x6"),
         tol=F32_TOL, **kw)
    if form in ("split_k", "reduce"):
        z, red = (3, True) if form == "reduce" else (1, False)
        S = gemm_hip._splits9f(shape[0], shape[1], shape[2], z, red)
        n = gemm_hip._lib.vfm_gemm9_workspace_floats(*shape, z, S, int(red))
        ws = [v for v, _, _ in scratch.items if v.dtype == F32]
        assert S > 1 and n > 0 and len(ws) == 1 and ws[0].numel() == n


def test_g9f_declines_activation_and_beta(scratch, g9f):
    """The piece form has plain / bias epilogues only: a product with an activation or beta != 0 is routed to
    gemm8's f32x6 form (its region says so), with the right values."""
    _run(scratch, F32, 304, 264, 64, a_kc=True, b_kc=False, pitched=True, route=("g8", 0), bias_dim=1, act="gelu",
         alpha=0.75, expect=_g8_region(F32, True, False), tol=F32_TOL)
    _run(scratch, F32, 304, 264, 64, a_kc=True, b_kc=False, pitched=True, route=("g8", 0), alpha=0.5, beta=-2.0,
         expect=_g8_region(F32, True, False), tol=F32_TOL, seed=1)


# ------------------------------------------------------------------------------------------------------------------
# the exact-fp32 kernel (csrc/sgemm.hip, vfm_sgemm)

def _sg_region(a_kc, b_kc, tile=None):
    if tile is None:
        return f"sgemm<{_tb(a_kc)},{_tb(b_kc)},"
    bm, bn = gemm_hip.SG_TILES[tile & 3]
    return f"sgemm<{_tb(a_kc)},{_tb(b_kc)},{bm},{bn},{1 + (tile >> 2)}>"


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_sgemm_scalar_load_path(scratch, a_kc, b_kc, pitched):
    """(10, 12, 7): contiguous extents / leading dims that are not multiples of 4 floats: bounds-checked scalar
    staging next to the poison."""
    _run(scratch, F32, 10, 12, 7, a_kc=a_kc, b_kc=b_kc, pitched=pitched, call="sgemm", expect=_sg_region(a_kc, b_kc),
         tol=SGEMM_TOL)


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("tile", range(8))
def test_sgemm_tiles(scratch, tile, a_kc, b_kc, pitched):
    """Each tile code (and + 4: two wave groups over K) forced at (136, 72, 100): ragged in M, N and the 32-deep K."""
    _run(scratch, F32, 136, 72, 100, a_kc=a_kc, b_kc=b_kc, pitched=pitched, call="sgemm", tile=tile, splits=1,
         n_scratch=0, expect=_sg_region(a_kc, b_kc, tile), tol=SGEMM_TOL)


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("form", ["planned_splits", "shared_a", "shared_b", "reduce", "fold", "fold_pitched_out"])
def test_sgemm_split_batch_reduce_fold(scratch, form, a_kc, b_kc):
    """(40, 40, 4096) with the planned K splits, batch-shared operands, the batch reduction (partials in an
    embedded workspace of exactly vfm_sgemm_workspace_floats) and the batch-folded narrow planes N = 16, z = 5
    (folded only for a dense out and N-contiguous B; the pitched out runs the batched form)."""
    shape, kw = (136, 72, 100), dict(pitched=True)
    if form == "planned_splits":
        shape = (40, 40, 4096)
        S = gemm_hip._sg_plan(40, 40, 4096, 1, 128)[1]
        assert S > 1
        kw.update(n_scratch=1)
    elif form.startswith("shared"):
        kw.update(z=3, shared=form[-1].upper())
    elif form == "reduce":
        kw.update(z=3, reduce_batch=True, n_scratch=1)
    else:
        shape = (136, 16, 100)
        kw.update(z=5, shared="A", dense_out=(form == "fold"), splits=1)
    _run(scratch, F32, *shape, a_kc=a_kc, b_kc=b_kc, call="sgemm", expect=_sg_region(a_kc, b_kc), tol=SGEMM_TOL, **kw)
    if form == "planned_splits":
        assert scratch.items[0][0].numel() == gemm_hip._lib.vfm_sgemm_workspace_floats(40, 40, 1, S, 0)
    elif form == "reduce":
        S = gemm_hip._sg_plan(136, 72, 100, 1, 3 * 4)[1]
        assert scratch.items[0][0].numel() == max(1, gemm_hip._lib.vfm_sgemm_workspace_floats(136, 72, 3, S, 1))


@pytest.mark.parametrize("bias_dim,act", [(0, "gelu_tanh"), (1, "gelu")])
@pytest.mark.parametrize("splits", [1, 3])
def test_sgemm_epilogue(scratch, bias_dim, act, splits):
    _run(scratch, F32, 136, 72, 100, a_kc=True, b_kc=False, pitched=True, call="sgemm", bias_dim=bias_dim, act=act,
         alpha=0.75, z=2, shared="A", splits=splits, expect=_sg_region(True, False), tol=SGEMM_TOL)


@pytest.mark.parametrize("splits", [1, 3])
def test_sgemm_beta_accumulates_inside_pitched_out(scratch, splits):
    _run(scratch, F32, 136, 72, 100, a_kc=True, b_kc=True, pitched=True, call="sgemm", z=2, alpha=0.5, beta=-2.0,
         splits=splits, expect=_sg_region(True, True), tol=SGEMM_TOL)


# ------------------------------------------------------------------------------------------------------------------
# the batch-folded product (csrc/gemm.hip, vfm_gemm_fold)

@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("a_kc", [True, False])
@pytest.mark.parametrize("epi", ["plain", "bias_act_alpha", "beta"])
def test_gemm_fold(scratch, monkeypatch, a_kc, pitched, epi):
    """(O, I, P, Bn) = (200, 136, 16, 9): shared A against per-sample planes of 16 columns as one product over
    N = 9 x 16; the planes' pitch and the out's plane gap keep their fill."""
    monkeypatch.setattr(gemm_hip, "FOLD", True)
    kw = dict(bias_dim=0, act="gelu_tanh", alpha=0.75) if epi == "bias_act_alpha" else \
        (dict(alpha=0.5, beta=-2.0) if epi == "beta" else {})
    _run(scratch, F32, 200, 16, 136, z=9, shared="A", a_kc=a_kc, b_kc=False, pitched=pitched, auto=True, n_scratch=0,
         expect=f"gemm_fold<f32x6,{_tb(a_kc)},true>", tol=F32_TOL, **kw)
