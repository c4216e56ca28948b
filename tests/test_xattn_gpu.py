"""Masked short-key attention kernels (csrc/xattn.hip) on cuda:0.

  * vfm_cross_attention_f32_fwd / _bwd against a float64 torch evaluation of the reference formula (cat the null
    key / value, boolean mask, softmax, P.V; reference networks/utils/gigagan_utils.py:94-146), forward and all
    five gradients (dq, dk, dv, dnull_k, dnull_v; dk / dv are the two halves of the packed dkv). Criterion, per
    tensor, tests/test_attention_f32_gpu.py's: rel(kernel, f64) <= 2 rel(torch fp32 math, f64) + 1e-6 with
    rel = max |err| / max |ref|. Nq 160 is a ragged second query tile (and a second dK / dV chunk), L 5 is fewer
    keys than one MFMA block, L 64 gives 65 keys (one past a 64-key tile).
  * exactness: mask of ones == no mask bitwise; the k / v rows of masked keys do not matter bitwise; their dkv rows
    are exact zeros; two runs agree bitwise; NaN-prefilled outputs come back fully written.
  * vfm_attention_keymask_fwd against float64 SDPA on the bf16-rounded inputs with tests/test_qwen_gpu.py's bounds
    for the same arithmetic (max |err| <= 1.5e-2 m, mean |err| <= 2e-3 m, m = max |ref|).
  * the CrossAttention module: VFM_XATTN=hip against the torch formulation and float64.
A row with no valid key is outside the kernels' contract and is not exercised.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _mask(kind, B, L):
    if kind == "none":
        return None
    m = torch.ones(B, L, dtype=torch.bool)
    if kind == "lengths":                    # [1, L, 1, L, ...]
        for b in range(0, B, 2):
            m[b, 1:] = False
    elif kind == "holes":                    # every third key off (and a different phase per sample)
        for b in range(B):
            m[b, (b + 1) % 3::3] = False
    return m.to(DEV)


def _inputs(B, H, Nq, L, d, seed, qscale=1.0):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Nq, H, d, generator=g) * qscale).to(DEV)
    kv = torch.randn(B, L, 2, H, d, generator=g).to(DEV)
    null_kv = torch.randn(2, H, d, generator=g).to(DEV)
    do = torch.randn(B, Nq, H, d, generator=g).to(DEV)
    return q, kv, null_kv, do


def _formula(q, kv, null_kv, mask, mask_null, do, dtype):
    """cat null, boolean mask, softmax, P.V in `dtype`; returns o and the gradients (dq, dkv, dnull)."""
    q, kv, null_kv = (t.detach().to(dtype).requires_grad_(True) for t in (q, kv, null_kv))
    B, Nq, H, d = q.shape
    k, v = kv[:, :, 0], kv[:, :, 1]                                       # [B, L, H, d]
    k = torch.cat([null_kv[0][None, None].expand(B, 1, H, d), k], 1)
    v = torch.cat([null_kv[1][None, None].expand(B, 1, H, d), v], 1)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * d ** -0.5
    if mask is not None:
        first = torch.full((B, 1), not mask_null, dtype=torch.bool, device=mask.device)
        full = torch.cat([first, mask], 1)
        s = s.masked_fill(~full[:, None, None, :], float("-inf"))
    o = torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v)
    o.backward(do.to(dtype))
    return o.detach(), q.grad, kv.grad, null_kv.grad


def _ours(q, kv, null_kv, mask, mask_null, do):
    from torch_utils.ops import xattn_hip
    q, kv, null_kv = (t.detach().clone().requires_grad_(True) for t in (q, kv, null_kv))
    o = xattn_hip.cross_attention_core(q, kv, null_kv, mask, mask_null)
    o.backward(do)
    return o.detach(), q.grad, kv.grad, null_kv.grad


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


NAMES = ("o", "dq", "dkv", "dnull")


def _check(q, kv, null_kv, mask, mask_null, do, tag):
    ref = _formula(q, kv, null_kv, mask, mask_null, do, torch.float64)
    t32 = _formula(q, kv, null_kv, mask, mask_null, do, torch.float32)
    ours = _ours(q, kv, null_kv, mask, mask_null, do)
    report, bad = [], []
    for name, x, y, r in zip(NAMES, ours, t32, ref):
        if float(r.abs().max()) == 0.0:                     # dnull when the null key is masked: exact zeros
            assert not x.any(), name
            continue
        e, et = _rel(x, r), _rel(y, r)
        report.append(f"{name} {e:.2e} (torch {et:.2e})")
        if not e <= 2 * et + 1e-6:
            bad.append(name)
    print(f"{tag}: " + ", ".join(report))
    assert not bad, (bad, report)
    return ours


@pytest.mark.parametrize("kind", ["none", "ones", "lengths", "holes"])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("L", [5, 64])
@pytest.mark.parametrize("Nq", [64, 160])
def test_cross_attention_kernel_matches_float64(Nq, L, d, kind):
    B, H = 2, 2
    q, kv, null_kv, do = _inputs(B, H, Nq, L, d, seed=Nq + L + d)
    mask = _mask(kind, B, L)
    ours = _check(q, kv, null_kv, mask, False, do, f"Nq{Nq} L{L} d{d} {kind}")
    if mask is not None:
        dead = ~mask[:, :, None, None, None].expand_as(ours[2])
        assert not ours[2][dead].any(), "dkv rows of masked keys must be exact zeros"


@pytest.mark.parametrize("kind", ["lengths", "holes"])
def test_cross_attention_kernel_null_masked_with_the_mask(kind):
    """mask_null: the reference module's own rule (a False column is prepended to the mask), so dnull is zero."""
    B, H, Nq, L, d = 2, 2, 160, 64, 64
    q, kv, null_kv, do = _inputs(B, H, Nq, L, d, seed=11)
    ours = _check(q, kv, null_kv, _mask(kind, B, L), True, do, f"mask_null {kind}")
    assert not ours[3].any()


def test_cross_attention_kernel_large_scores():
    """Scores of magnitude ~50 (as test_attention_f32_packed_qkv_large_scores): the softmax statistics."""
    B, H, Nq, L, d = 2, 2, 160, 64, 64
    q, kv, null_kv, do = _inputs(B, H, Nq, L, d, seed=3, qscale=50.0)
    s = torch.einsum("bqhd,bkhd->bhqk", q, kv[:, :, 0]) * d ** -0.5
    assert float(s.abs().max()) > 50
    _check(q, kv, null_kv, _mask("holes", B, L), False, do, "large scores")


def test_cross_attention_kernel_f32x3_opt_in(monkeypatch):
    from torch_utils import custom_ops
    monkeypatch.setattr(custom_ops, "F32_PRODUCTS", "f32x3")
    B, H, Nq, L, d = 2, 2, 160, 64, 64
    q, kv, null_kv, do = _inputs(B, H, Nq, L, d, seed=4)
    mask = _mask("holes", B, L)
    ref = _formula(q, kv, null_kv, mask, False, do, torch.float64)
    ours = _ours(q, kv, null_kv, mask, False, do)
    for x, r, t in zip(ours, ref, (5e-5, 2e-4, 2e-4, 2e-4)):     # test_attention_f32_gpu.py's f32x3 bounds
        assert _rel(x, r) < t, (_rel(x, r), t)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("Nq,L,d", [(160, 64, 64), (64, 5, 32)])
def test_cross_attention_kernel_exactness(Nq, L, d):
    from torch_utils.ops import xattn_hip
    B, H = 2, 2
    q, kv, null_kv, do = _inputs(B, H, Nq, L, d, seed=7 + L)
    # ones == none, bitwise
    a = _ours(q, kv, null_kv, None, False, do)
    b = _ours(q, kv, null_kv, _mask("ones", B, L), False, do)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(_bits(x), _bits(y)), name
    # two runs agree bitwise
    for name, x, y in zip(NAMES, a, _ours(q, kv, null_kv, None, False, do)):
        assert torch.equal(_bits(x), _bits(y)), name
    # what sits in the rows of masked keys does not matter
    mask = _mask("holes", B, L)
    other = kv.clone()
    other[~mask] = (torch.randn(other[~mask].shape, generator=torch.Generator().manual_seed(1)) * 7).to(DEV)
    assert not torch.equal(other, kv)
    a = _ours(q, kv, null_kv, mask, False, do)
    b = _ours(q, other, null_kv, mask, False, do)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert torch.equal(_bits(a[2][mask]), _bits(b[2][mask])) and torch.equal(_bits(a[3]), _bits(b[3]))
    assert not a[2][~mask].any() and not b[2][~mask].any()
    # NaN-prefilled outputs come back fully written
    nan = float("nan")
    o = torch.full((B, Nq, H, d), nan, device=DEV)
    o, lse = xattn_hip._core_fwd(q, kv, null_kv, mask, False, o=o)
    dq, dkv, dnull = xattn_hip._core_bwd(q, kv, null_kv, mask, False, o, do, lse, dq=torch.full_like(q, nan),
                                         dkv=torch.full_like(kv, nan), dnull=torch.full_like(null_kv, nan))
    for name, t in zip(("o", "lse", "dq", "dkv", "dnull"), (o, lse, dq, dkv, dnull)):
        assert not torch.isnan(t).any(), name
    assert torch.equal(_bits(o), _bits(a[0])) and torch.equal(_bits(dkv), _bits(a[2]))


def test_cross_attention_kernel_rejects_what_it_does_not_take():
    from torch_utils import custom_ops
    lib = custom_ops.get_native()
    assert lib.vfm_cross_attention_f32_workspace_floats(2, 2, 64, 128, 64) == custom_ops.VFM_NO_KERNEL   # 129 keys
    assert lib.vfm_cross_attention_f32_workspace_floats(2, 2, 64, 64, 48) == custom_ops.VFM_NO_KERNEL
    assert lib.vfm_cross_attention_f32_workspace_floats(2, 2, 0, 64, 64) == -2
    q, kv, null_kv, _ = _inputs(2, 2, 64, 128, 64, seed=0)
    o, lse = torch.empty_like(q), torch.empty(2, 2, 64, device=DEV)
    s = custom_ops.strides_of([q.stride(0), q.stride(1), q.stride(2)])
    rc = lib.vfm_cross_attention_f32_fwd(q.data_ptr(), kv.data_ptr(), null_kv.data_ptr(), None, o.data_ptr(),
                                         lse.data_ptr(), 2, 2, 64, 128, 64, s, s, 0.125, 0, 0,
                                         custom_ops.stream_ptr(DEV))
    assert rc == custom_ops.VFM_NO_KERNEL


# ------------------------------------------------------------------------------------------------ kernel (a)

def _km_inputs(B, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, 3 * H * 64, generator=g).to(torch.bfloat16)


def _km_mask(N, lengths):
    if lengths is None:
        return None
    m = torch.zeros(len(lengths), N, dtype=torch.bool)
    for b, n in enumerate(lengths):
        m[b, :n] = True
    return m


def _km_ref(qkv, H, mask):
    B, N, _ = qkv.shape
    q, k, v = qkv.double().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    am = None if mask is None else mask[:, None, None, :]
    return F.scaled_dot_product_attention(q, k, v, attn_mask=am).transpose(1, 2).reshape(B, N, H * 64)


@pytest.mark.parametrize("masked", [True, False], ids=["lengths", "none"])
@pytest.mark.parametrize("N", [64, 40, 100])
def test_keymask_attention_matches_float64(N, masked):
    from torch_utils.ops import kernel_timer, xattn_hip
    B, H = 3, 2
    qkv = _km_inputs(B, N, H, seed=N)
    mask = _km_mask(N, [1, 7, N]) if masked else None
    out = torch.full((B, N, H, 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    kernel_timer.enable(True)
    got = xattn_hip.keymask_attention_packed(qkv.to(DEV), H, None if mask is None else mask.to(DEV), out=out)
    torch.cuda.synchronize()
    assert "attention_keymask_fwd<bf16,64>" in kernel_timer.summary()
    kernel_timer.enable(False)
    got = got.cpu()
    assert not torch.isnan(got.float()).any()
    ref = _km_ref(qkv, H, mask)
    err = (got.double() - ref).abs()
    m = float(ref.abs().max())
    print(f"N{N} {'lengths' if masked else 'none'}: max {float(err.max()) / m:.2e} mean {float(err.mean()) / m:.2e}")
    assert float(err.max()) <= 1.5e-2 * m and float(err.mean()) <= 2e-3 * m


def test_keymask_attention_masked_keys_do_not_matter():
    from torch_utils.ops import xattn_hip
    B, H, N = 3, 2, 64
    qkv = _km_inputs(B, N, H, seed=5)
    mask = _km_mask(N, [1, 7, N])
    other = qkv.clone().reshape(B, N, 3, H * 64)
    fresh = (torch.randn(B, N, 2, H * 64, generator=torch.Generator().manual_seed(6)) * 3).to(torch.bfloat16)
    other[:, :, 1:][~mask] = fresh[~mask]                 # K and V of the masked keys
    other = other.reshape(B, N, -1)
    assert not torch.equal(other, qkv)
    a = xattn_hip.keymask_attention_packed(qkv.to(DEV), H, mask.to(DEV))
    b = xattn_hip.keymask_attention_packed(other.to(DEV), H, mask.to(DEV))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_keymask_attention_rejects_other_shapes():
    from torch_utils import custom_ops
    lib = custom_ops.get_native()
    for N, d in ((64, 80), (129, 64)):
        x = torch.zeros(1, N, 1, d, dtype=torch.bfloat16, device=DEV)
        s = custom_ops.strides_of([x.stride(0), x.stride(1), x.stride(2)])
        rc = lib.vfm_attention_keymask_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 1, 1, N, d,
                                           s, s, s, s, 0.125, custom_ops.stream_ptr(DEV))
        assert rc == custom_ops.VFM_NO_KERNEL, (N, d, rc)


# ------------------------------------------------------------------------------------------------ the module

class _Ops(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


def _module_run(module, fmap, context, mask, dy, dtype, device):
    import copy
    m = copy.deepcopy(module).to(device=device, dtype=dtype)
    x = fmap.to(device=device, dtype=dtype).requires_grad_(True)
    c = context.to(device=device, dtype=dtype).requires_grad_(True)
    y = m(x, c, mask=None if mask is None else mask.to(device))
    y.backward(dy.to(device=device, dtype=dtype))
    out = {"y": y.detach(), "dfmap": x.grad, "dcontext": c.grad}
    out.update({"d" + n: p.grad for n, p in m.named_parameters()})
    return out


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
def test_cross_attention_module_hip_against_torch(masked, monkeypatch):
    """dim 64, 2 heads of 32, 8 x 8 feature map, 64 text tokens, det_init weights (to_out is zero-initialised by
    default: the branch would be a no-op): the hip route and the torch formulation against float64."""
    from det_init import det_init
    from networks.utils.gigagan_utils import CrossAttention
    from torch_utils.ops import kernel_timer, xattn_hip
    B, dim, L, Dc = 2, 64, 64, 96
    module = CrossAttention(dim=dim, dim_context=Dc, dim_head=32, heads=2)
    det_init(module)
    g = torch.Generator().manual_seed(2)
    fmap, context = torch.randn(B, dim, 8, 8, generator=g), torch.randn(B, L, Dc, generator=g)
    dy = torch.randn(B, dim, 8, 8, generator=g)
    mask = _km_mask(L, [9, L]) if masked else None
    ref = _module_run(module, fmap, context, mask, dy, torch.float64, "cpu")
    monkeypatch.setattr(xattn_hip, "OWN", "torch")
    rec_t = _Ops()
    with rec_t:
        tor = _module_run(module, fmap, context, mask, dy, torch.float32, DEV)
    assert any(n.startswith("aten._scaled_dot_product") for n in rec_t.names)
    monkeypatch.setattr(xattn_hip, "OWN", "hip")
    kernel_timer.enable(True)
    rec = _Ops()
    with rec:
        hip = _module_run(module, fmap, context, mask, dy, torch.float32, DEV)
    torch.cuda.synchronize()
    seen = list(kernel_timer.summary())
    kernel_timer.enable(False)
    assert any(k.startswith("cross_attention_fwd<") for k in seen), seen
    assert any(k.startswith("cross_attention_bwd<") for k in seen), seen
    # no concatenation, no library attention and no library GEMM: every product of the Function is on gemm_hip
    hits = [n for n in rec.names if n.startswith(("aten.cat", "aten._scaled_dot_product", "aten.mm", "aten.bmm",
                                                  "aten.addmm", "aten.baddbmm", "aten.matmul"))]
    assert not hits, hits
    assert set(hip) == set(ref) == set(tor)
    report, bad = [], []
    for name in sorted(ref):
        r = ref[name]
        if float(r.abs().max()) == 0.0:                     # dnull_kv under a mask
            assert not hip[name].any(), name
            continue
        e, et = _rel(hip[name].cpu(), r), _rel(tor[name].cpu(), r)
        report.append(f"{name} {e:.2e} (torch {et:.2e})")
        if not e <= 2 * et + 1e-6:
            bad.append(name)
    print(", ".join(report))
    assert not bad, (bad, report)
