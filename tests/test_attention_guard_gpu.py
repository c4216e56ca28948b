"""Guard bands around the attention kernels (csrc/attention.hip, attention_f32.hip, xattn.hip, qwen.hip): no
stray reads that reach a stored value, no stray writes.

Every input is a view embedded in NaN (tests/guard_bands.py: base 16-B but not 512-B aligned, pitched where
the entry takes strides), every output a view embedded in a finite sentinel and pre-filled with NaN. A key row
past Nk, a query row past Nq or a value past a segment end that reaches the result -- even multiplied by a
zero probability -- turns it NaN; an output row or statistic stored past its extent changes the sentinel.
Parity is checked at the tolerances of the files that already test each kernel:
  attention (bf16)            tests/test_attention_gpu.py    max |err| <= 1.5e-2 m, mean |err| <= 2e-3 m, m = max |ref|
  attention_f32 fwd / bwd     tests/test_attention_f32_gpu.py 1e-5 on O, 5e-5 on dQ / dK / dV (f32x3: 5e-5 / 2e-4)
  cross attention fwd / bwd   tests/test_xattn_gpu.py         rel <= 2 rel(torch fp32) + 1e-6 (f32x3: 5e-5 / 2e-4)
  keymask attention, varlen   tests/test_xattn_gpu.py, tests/test_qwen_gpu.py: the bf16 bounds above
lse (base-2 logsumexp of the scaled scores) shares O's bound: it is O's normaliser. delta = sum_d dO O is an fp32
sum of d products of the kernel's own O: within (d + 1) 2^-24 sum |dO O| of the fp64 sum over that O."""
import math

import pytest
import torch
import torch.nn.functional as F

import guard_bands as gb
from torch_utils import custom_ops
from torch_utils.ops import attn_hip, kernel_timer, qwen_hip, xattn_hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_lib = custom_ops.get_native()


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


def _nan_out(shape, dtype=torch.float32, **kw):
    """A sentinel-embedded output view, NaN inside."""
    return gb.embed(torch.full(shape, gb.POISON, dtype=dtype, device=DEV), fill=gb.SENTINEL, **kw)


def _assert_guards(guards):
    torch.cuda.synchronize()
    for what, views, buf, fill in guards:
        assert gb.intact(views, buf, fill), f"{what}: " + gb.describe(views, buf, fill)


def _assert_written(**outs):
    for name, t in outs.items():
        assert not torch.isnan(t.float()).any(), f"{name}: {int(torch.isnan(t.float()).sum())} NaN (unwritten or poisoned)"


def _bf16_bounds(out, ref, tag):
    err = (out.double() - ref.double()).abs()
    m = float(ref.abs().max())
    print(f"{tag}: max {float(err.max()) / m:.2e} mean {float(err.mean()) / m:.2e} of max|ref|")
    assert float(err.max()) <= 1.5e-2 * m, (float(err.max()), m)
    assert float(err.mean()) <= 2e-3 * m, (float(err.mean()), m)


def _s(t):
    return custom_ops.strides_of([t.stride(0), t.stride(1), t.stride(2)])


# ------------------------------------------------------------------------------------------------ bf16 towers

@pytest.mark.parametrize("N", [1, 65, 130])
def test_attention_bf16_packed_views(N):
    """attn_hip.attention on q / k / v views of one NaN-embedded packed [B, N, 3, H, 64] and an out view whose
    token stride is larger than H * 64."""
    B, H = 2, 3
    g = torch.Generator().manual_seed(N)
    packed, pbuf = gb.embed(torch.randn(B, N, 3, H, 64, generator=g).to(torch.bfloat16).to(DEV), fill=gb.POISON)
    q, k, v = packed.unbind(2)
    out, obuf = _nan_out((B, N, H, 64), torch.bfloat16, gap=64)
    assert out.stride(1) == H * 64 + 64 and q.data_ptr() % 512 == 16
    kernel_timer.enable(True)
    try:
        res = attn_hip.attention(q, k, v, out=out)
        names = list(kernel_timer.summary())
    finally:
        kernel_timer.enable(False)
    assert names == ["attention_fwd<bf16,64>"], names
    _assert_guards([("qkv", [q, k, v], pbuf, gb.POISON), ("out", out, obuf, gb.SENTINEL)])
    assert res.data_ptr() == out.data_ptr()
    _assert_written(out=out)
    qd, kd, vd = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qd, kd, vd).permute(0, 2, 1, 3)
    _bf16_bounds(out, ref, f"attention N{N}")


@pytest.mark.parametrize("N,lengths", [(64, [1, 63, 64, 64]), (100, [1, 63, 64, 100])])
def test_keymask_attention_guarded(N, lengths):
    """xattn_hip.keymask_attention_packed(out=): masks whose valid length is 1, 63, 64 and all keys. The mask buffer
    is embedded in `attend`, so a mask byte read past [B, N] would unmask a key; the keys past N are NaN."""
    B, H = len(lengths), 2
    g = torch.Generator().manual_seed(N)
    qkv, qbuf = gb.embed(torch.randn(B, N, 3 * H * 64, generator=g).to(torch.bfloat16).to(DEV), fill=gb.POISON)
    m = torch.zeros(B, N, dtype=torch.bool)
    for b, n in enumerate(lengths):
        m[b, :n] = True
    mask, mbuf = gb.embed(m.to(DEV), fill=True)
    out, obuf = _nan_out((B, N, H, 64), torch.bfloat16, gap=64)
    kernel_timer.enable(True)
    try:
        res = xattn_hip.keymask_attention_packed(qkv, H, mask, out=out)
        names = list(kernel_timer.summary())
    finally:
        kernel_timer.enable(False)
    assert names == ["attention_keymask_fwd<bf16,64>"], names
    _assert_guards([("qkv", qkv, qbuf, gb.POISON), ("mask", mask, mbuf, True), ("out", out, obuf, gb.SENTINEL)])
    assert res.data_ptr() == out.data_ptr() and res.shape == (B, N, H * 64)
    _assert_written(out=out)
    q, k, v = qkv.double().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=mask[:, None, None, :]).transpose(1, 2)
    _bf16_bounds(out, ref, f"keymask N{N}")


# ------------------------------------------------------------------------------------------------ fp32 attention

def _ref_attention(q, k, v, do):
    """fp64 softmax(q k^T / sqrt(d)) v on [B, N, H, d] operands -> o, lse (base 2), dq, dk, dv."""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * q.shape[-1] ** -0.5
    o = torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v)
    o.backward(do.double())
    return o.detach(), (torch.logsumexp(s, -1) / math.log(2.0)).detach(), q.grad, k.grad, v.grad


def _attention32_guarded(q, k, v, in_guards, do, grads=None):
    """vfm_attention_f32_fwd / _bwd as attn_hip._Attention32 calls them, on embedded operands; `grads`: (dq, dk, dv,
    guard entries) views to write (packed form), default three pitched embedded tensors."""
    B, Nq, H, d = q.shape
    Nk = k.shape[1]
    pitch = dict(pitch=d + 4, gap=8)
    o, obuf = _nan_out((B, Nq, H, d), **pitch)
    lse, lbuf = _nan_out((B, H, Nq))
    delta, dbuf = _nan_out((B, H, Nq))
    guards = list(in_guards) + [("o", o, obuf, gb.SENTINEL), ("lse", lse, lbuf, gb.SENTINEL),
                                ("delta", delta, dbuf, gb.SENTINEL)]
    if grads is None:
        (dq, qb), (dk, kb), (dv, vb) = (_nan_out(t.shape, **pitch) for t in (q, k, v))
        guards += [("dq", dq, qb, gb.SENTINEL), ("dk", dk, kb, gb.SENTINEL), ("dv", dv, vb, gb.SENTINEL)]
    else:
        dq, dk, dv, extra = grads
        guards += extra
    for t in (q, k, v, o, do, dq, dk, dv):
        assert attn_hip._s4(t) is not None and t.data_ptr() % 512 != 0          # readable in place, 16-B aligned only
    prec, _, tag = custom_ops.f32_precision()
    st = custom_ops.stream_ptr(DEV)
    kernel_timer.enable(True)
    try:
        with kernel_timer.region(f"attention_fwd<{tag},{d}>"):
            rc = _lib.vfm_attention_f32_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H,
                                            Nq, Nk, d, _s(q), _s(k), _s(v), _s(o), float(d) ** -0.5, prec, st)
        assert rc == 0, rc
        with kernel_timer.region(f"attention_bwd<{tag},{d}>"):
            rc = _lib.vfm_attention_f32_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(),
                                            lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                            dv.data_ptr(), B, H, Nq, Nk, d, _s(q), _s(k), _s(v), _s(o), _s(do), _s(dq),
                                            _s(dk), _s(dv), float(d) ** -0.5, prec, st)
        assert rc == 0, rc
        names = sorted(kernel_timer.summary())
    finally:
        kernel_timer.enable(False)
    assert names == [f"attention_bwd<{tag},{d}>", f"attention_fwd<{tag},{d}>"], names     # both launched kernels
    _assert_guards(guards)
    _assert_written(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)
    ro, rlse, rdq, rdk, rdv = _ref_attention(q, k, v, do)
    t_o, t_g = (5e-5, 2e-4) if tag == "f32x3" else (1e-5, 5e-5)
    errs = {"o": (_rel(o, ro), t_o), "lse": (_rel(lse, rlse), t_o), "dq": (_rel(dq, rdq), t_g),
            "dk": (_rel(dk, rdk), t_g), "dv": (_rel(dv, rdv), t_g)}
    print(f"{tag} d{d} Nq{Nq} Nk{Nk}: " + ", ".join(f"{n} {e:.2e}" for n, (e, _) in errs.items()))
    for n, (e, t) in errs.items():
        assert e < t, (n, e, t)
    prod = do.double() * o.double()
    dref, dbound = prod.sum(-1).permute(0, 2, 1), prod.abs().sum(-1).permute(0, 2, 1) * (d + 1) * 2.0 ** -24
    assert bool(((delta.double() - dref).abs() <= dbound + 1e-30).all())


def _embed32(t):
    return gb.embed(t.to(DEV), fill=gb.POISON, pitch=t.shape[-1] + 4, gap=8)


@pytest.fixture(params=["f32x6", "f32x3"])
def precision(request, monkeypatch):
    monkeypatch.setattr(custom_ops, "F32_PRODUCTS", request.param)
    assert custom_ops.f32_precision()[2] == request.param
    return request.param


@pytest.mark.parametrize("Nq,Nk", [(37, 5), (70, 65), (130, 129)])
@pytest.mark.parametrize("d", [64, 32])
def test_attention_f32_separate_views(precision, d, Nq, Nk):
    """q, k, v, dO: separate NaN-embedded token-major views (head rows of d + 4 floats, 8 more between tokens);
    o, lse, delta, dq, dk, dv sentinel-embedded."""
    B, H = 2, 2
    g = torch.Generator().manual_seed(Nq * 7 + Nk + d)
    (q, qb), (k, kb), (v, vb), (do, db) = (_embed32(torch.randn(B, n, H, d, generator=g)) for n in (Nq, Nk, Nk, Nq))
    _attention32_guarded(q, k, v, [("q", q, qb, gb.POISON), ("k", k, kb, gb.POISON), ("v", v, vb, gb.POISON),
                                   ("do", do, db, gb.POISON)], do)


@pytest.mark.parametrize("d", [64, 32])
def test_attention_f32_null_key_cat(precision, d):
    """The decoder's null key / value: Nk = Nq + 1 (one key past a 64-key tile), k and v views of an embedded cat."""
    B, H, Nq = 2, 2, 64
    g = torch.Generator().manual_seed(d)
    q, qb = _embed32(torch.randn(B, Nq, H, d, generator=g))
    do, db = _embed32(torch.randn(B, Nq, H, d, generator=g))
    nk = torch.randn(1, 1, H, d, generator=g).expand(B, 1, H, d)
    k, kb = _embed32(torch.cat([nk, torch.randn(B, Nq, H, d, generator=g)], 1))
    v, vb = _embed32(torch.cat([nk * 0.5, torch.randn(B, Nq, H, d, generator=g)], 1))
    _attention32_guarded(q, k, v, [("q", q, qb, gb.POISON), ("k", k, kb, gb.POISON), ("v", v, vb, gb.POISON),
                                   ("do", do, db, gb.POISON)], do)


@pytest.mark.parametrize("d,N", [(64, 70), (32, 130)])
def test_attention_f32_packed_qkv(precision, d, N):
    """The adapter's packed projection: q, k, v = qkv.unbind(2) of one NaN-embedded [B, N, 3, H, d]; dq, dk, dv =
    dqkv.unbind(2) of one sentinel-embedded buffer (attn_hip._Attention32Packed's layout)."""
    B, H = 2, 2
    g = torch.Generator().manual_seed(N + d)
    qkv, qbuf = gb.embed(torch.randn(B, N, 3, H, d, generator=g).to(DEV), fill=gb.POISON)
    do, db = _embed32(torch.randn(B, N, H, d, generator=g))
    dqkv, gbuf = _nan_out((B, N, 3, H, d))
    q, k, v = qkv.unbind(2)
    dq, dk, dv = dqkv.unbind(2)
    _attention32_guarded(q, k, v, [("qkv", [q, k, v], qbuf, gb.POISON), ("do", do, db, gb.POISON)], do,
                         grads=(dq, dk, dv, [("dqkv", [dq, dk, dv], gbuf, gb.SENTINEL)]))
    _assert_written(dqkv=dqkv)


# ------------------------------------------------------------------------------------------------ cross attention

def _xattn_formula(q, kv, null_kv, mask, mask_null, do, dtype):
    """tests/test_xattn_gpu.py's restatement: cat null, boolean mask, softmax, P.V in `dtype` -> o, lse (base 2),
    dq, dkv, dnull."""
    q, kv, null_kv = (t.detach().to(dtype).requires_grad_(True) for t in (q, kv, null_kv))
    B, Nq, H, d = q.shape
    k = torch.cat([null_kv[0][None, None].expand(B, 1, H, d), kv[:, :, 0]], 1)
    v = torch.cat([null_kv[1][None, None].expand(B, 1, H, d), kv[:, :, 1]], 1)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * d ** -0.5
    first = torch.full((B, 1), not mask_null, dtype=torch.bool, device=mask.device)
    s = s.masked_fill(~torch.cat([first, mask], 1)[:, None, None, :], float("-inf"))
    o = torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v)
    o.backward(do.to(dtype))
    return o.detach(), (torch.logsumexp(s, -1) / math.log(2.0)).detach(), q.grad, kv.grad, null_kv.grad


def _xattn_guarded(L, Nq, d, mask_null, monkeypatch):
    B, H = 2, 2
    g = torch.Generator().manual_seed(L * 1000 + Nq + d + int(mask_null))
    q, qb = _embed32(torch.randn(B, Nq, H, d, generator=g))
    do, db = _embed32(torch.randn(B, Nq, H, d, generator=g))
    kv, kvb = gb.embed(torch.randn(B, L, 2, H, d, generator=g).to(DEV), fill=gb.POISON)
    null_kv, nb = gb.embed(torch.randn(2, H, d, generator=g).to(DEV), fill=gb.POISON)
    m = torch.ones(B, L, dtype=torch.bool)
    m[1, max(1, L // 3):] = False                              # sample 1: a third of the keys (L = 1: its one key)
    m[0, 2::5] = False                                         # sample 0: holes
    mask, mb = gb.embed(m.to(DEV), fill=True)                  # the fill would unmask a key past [B, L]
    o, ob = _nan_out((B, Nq, H, d), pitch=d + 4, gap=8)
    lse, lb = _nan_out((B, H, Nq))
    dq, dqb = _nan_out((B, Nq, H, d), pitch=d + 4, gap=8)
    dkv, dkvb = _nan_out((B, L, 2, H, d))
    dnull, dnb = _nan_out((2, H, d))
    made = []

    def workspace(B_, H_, Nq_, L_, d_, device):
        n = _lib.vfm_cross_attention_f32_workspace_floats(B_, H_, Nq_, L_, d_)
        assert n > 0
        made.append(_nan_out((n,)))
        return made[-1][0]

    monkeypatch.setattr(xattn_hip, "_workspace", workspace)
    prec, _, tag = custom_ops.f32_precision()
    kernel_timer.enable(True)
    try:
        with kernel_timer.region(f"cross_attention_fwd<{tag},{d}>"):
            rc = _lib.vfm_cross_attention_f32_fwd(q.data_ptr(), kv.data_ptr(), null_kv.data_ptr(), mask.data_ptr(),
                                                  o.data_ptr(), lse.data_ptr(), B, H, Nq, L, d, _s(q), _s(o),
                                                  float(d) ** -0.5, int(mask_null), prec, custom_ops.stream_ptr(DEV))
        assert rc == 0, rc
        res = xattn_hip._core_bwd(q, kv, null_kv, mask, mask_null, o, do, lse, dq=dq, dkv=dkv, dnull=dnull)
        names = sorted(kernel_timer.summary())
    finally:
        kernel_timer.enable(False)
    assert names == [f"cross_attention_bwd<{tag},{d}>", f"cross_attention_fwd<{tag},{d}>"], names
    assert [t.data_ptr() for t in res] == [dq.data_ptr(), dkv.data_ptr(), dnull.data_ptr()]
    assert len(made) == 1
    _assert_guards([("q", q, qb, gb.POISON), ("do", do, db, gb.POISON), ("kv", kv, kvb, gb.POISON),
                    ("null_kv", null_kv, nb, gb.POISON), ("mask", mask, mb, True), ("o", o, ob, gb.SENTINEL),
                    ("lse", lse, lb, gb.SENTINEL), ("dq", dq, dqb, gb.SENTINEL), ("dkv", dkv, dkvb, gb.SENTINEL),
                    ("dnull", dnull, dnb, gb.SENTINEL), ("workspace", made[0][0], made[0][1], gb.SENTINEL)])
    _assert_written(o=o, lse=lse, dq=dq, dkv=dkv, dnull=dnull)
    # a second output view through the wrapper's own forward (o=) agrees bitwise with the C entry's
    o2, o2b = _nan_out((B, Nq, H, d), pitch=d + 4, gap=8)
    xattn_hip._core_fwd(q, kv, null_kv, mask, mask_null, o=o2)
    _assert_guards([("o (_core_fwd)", o2, o2b, gb.SENTINEL)])
    assert torch.equal(o2.view(torch.int32), o.view(torch.int32))
    ref = _xattn_formula(q, kv, null_kv, mask, mask_null, do, torch.float64)
    ours = (o, lse, dq, dkv, dnull)

    def zero_ref(n, x):
        """A gradient whose reference is exactly zero. dnull under a masked null key: exact zeros. dq with one valid
        key (L = 1, null masked): p = 1, so dS = p (dP - delta) = 0 analytically and the kernel stores the rounding
        residue of the two d-term fp32 sums dP and delta, each within (d + 1) 2^-24 sum |dO O| (V = O here), times
        scale |k|; twice that for the piece products' own dropped terms."""
        if n == "dnull":
            assert not x.any(), n
            return
        assert n == "dq", n
        S = (do.double() * o.double()).abs().sum(-1, keepdim=True)
        bound = 4 * (d + 1) * 2.0 ** -24 * S * d ** -0.5 * float(kv.abs().max())
        assert bool((x.double().abs() <= bound).all()), (n, float(x.abs().max()), float(bound.min()))

    names = ("o", "lse", "dq", "dkv", "dnull")
    if tag == "f32x3":
        for n, x, r, t in zip(names, ours, ref, (5e-5, 5e-5, 2e-4, 2e-4, 2e-4)):
            if float(r.abs().max()) == 0.0:
                zero_ref(n, x)
            else:
                assert _rel(x, r) < t, (n, _rel(x, r), t)
        return
    t32 = _xattn_formula(q, kv, null_kv, mask, mask_null, do, torch.float32)
    report, bad = [], []
    for n, x, y, r in zip(names, ours, t32, ref):
        if float(r.abs().max()) == 0.0:
            zero_ref(n, x)
            continue
        e, et = _rel(x, r), _rel(y, r)
        report.append(f"{n} {e:.2e} (torch {et:.2e})")
        if not e <= 2 * et + 1e-6:
            bad.append(n)
    print(f"L{L} Nq{Nq} d{d} mask_null{int(mask_null)}: " + ", ".join(report))
    assert not bad, (bad, report)
    dead = ~mask[:, :, None, None, None].expand_as(dkv)
    assert not dkv[dead].any(), "dkv rows of masked keys must be exact zeros"


@pytest.mark.parametrize("mask_null", [False, True])
@pytest.mark.parametrize("d", [64, 32])
@pytest.mark.parametrize("Nq", [37, 130])
@pytest.mark.parametrize("L", [1, 77])
def test_cross_attention_guarded(L, Nq, d, mask_null, monkeypatch):
    """vfm_cross_attention_f32_fwd (o, lse embedded) and xattn_hip._core_bwd(dq=, dkv=, dnull=) with the workspace
    substituted by an embedded one of exactly vfm_cross_attention_f32_workspace_floats floats."""
    _xattn_guarded(L, Nq, d, mask_null, monkeypatch)


def test_cross_attention_guarded_f32x3(monkeypatch):
    monkeypatch.setattr(custom_ops, "F32_PRODUCTS", "f32x3")
    _xattn_guarded(77, 130, 64, False, monkeypatch)


# ------------------------------------------------------------------------------------------------ varlen RoPE attention

def _rope_ref(qkv, cos, sin, lengths, heads, hd):
    """tests/test_qwen_gpu.py's fp64 restatement: per segment, the rotated q and k rounded to bf16 first."""
    T = qkv.shape[0]
    rot = lambda x: torch.cat((-x[..., hd // 2:], x[..., :hd // 2]), -1)
    q, k, v = qkv.double().reshape(T, 3, heads, hd).unbind(1)
    c, s = cos.double()[:, None], sin.double()[:, None]
    q = (q * c + rot(q) * s).to(torch.bfloat16).double()
    k = (k * c + rot(k) * s).to(torch.bfloat16).double()
    out = torch.empty(T, heads, hd, dtype=torch.float64, device=qkv.device)
    pos = 0
    for n in lengths:
        sl = slice(pos, pos + n)
        sc = torch.einsum("qhd,khd->hqk", q[sl], k[sl]) * hd ** -0.5
        out[sl] = torch.einsum("hqk,khd->qhd", sc.softmax(-1), v[sl])
        pos += n
    return out.reshape(T, heads * hd)


@pytest.mark.parametrize("hint", ["max", "unknown"])
def test_rope_attention_varlen_guarded(hint):
    """qwen_hip.rope_attention_varlen(out=): segments of 1, 63, 64 and 65 tokens (T = 193), qkv / cos / sin embedded
    in NaN and then in large finite values: the same bits either way (nothing past T, and nothing across a
    segment end, reaches a stored value), out sentinel-embedded."""
    heads, hd, lengths = 2, 80, [1, 63, 64, 65]
    T = sum(lengths)
    g = torch.Generator().manual_seed(T)
    qkv0 = torch.randn(T, 3 * heads * hd, generator=g).to(torch.bfloat16).to(DEV)
    ang = torch.rand(T, hd // 2, generator=g) * 40.0
    emb = torch.cat((ang, ang), -1)
    cos0, sin0 = emb.cos().to(DEV), emb.sin().to(DEV)
    cu = torch.tensor([0, 1, 64, 128, 193], dtype=torch.int32, device=DEV)
    max_len = 65 if hint == "max" else 0
    outs = []
    for fill in (gb.POISON, 1e30):
        (qkv, qb), (cos, cb), (sin, sb) = (gb.embed(t, fill=fill) for t in (qkv0, cos0, sin0))
        out, ob = _nan_out((T, heads * hd), torch.bfloat16)
        kernel_timer.enable(True)
        try:
            res = qwen_hip.rope_attention_varlen(qkv, cos, sin, cu, heads, max_len, out=out)
            names = list(kernel_timer.summary())
        finally:
            kernel_timer.enable(False)
        assert names == [f"rope_attention_varlen<bf16,80,{qwen_hip.attention_waves(max_len)}>"], names
        _assert_guards([("qkv", qkv, qb, fill), ("cos", cos, cb, fill), ("sin", sin, sb, fill),
                        ("out", out, ob, gb.SENTINEL)])
        assert res.data_ptr() == out.data_ptr()
        _assert_written(out=out)
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "the fill around the inputs reached the result"
    _bf16_bounds(outs[0], _rope_ref(qkv0, cos0, sin0, lengths, heads, hd), f"varlen {hint}")
