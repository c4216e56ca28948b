"""Kernels of the Qwen2.5-VL vision tower (csrc/qwen.hip) and the tower on them, on cuda:0.

  * varlen RoPE attention (head dim 80) against an fp64 torch reference on the same bf16 inputs that loops over the
    segments and rounds the rotated q and k to bf16. The arithmetic is csrc/attention.hip's (fp32 online softmax, P
    rounded to bf16, bf16 output), so the bounds are tests/test_attention_gpu.py's: max |err| <= 1.5e-2 max|ref|,
    mean |err| <= 2e-3 max|ref|. The output is poison-filled first, and no key may leak across segments: changing
    every other segment's K and V leaves a segment's output bitwise equal.
  * RMSNorm and SwiGLU rows against fp64 from the same inputs with the same rounding points: one bf16 ulp
    (|err| <= 2^-7 |ref| + floor) for the norm's single rounding, two for SwiGLU's two roundings; pad columns
    exactly zero. fp32 streams: 1e-5 relative (fp32 arithmetic against fp64).
  * the patch gather against the torch permutation, bitwise.
  * the tower against the reference's golden vectors: bf16 relative L2 <= 2 x the stored e_bf16 of that case and
    output (two independent bf16 evaluations of one fp32 function can differ by the sum of their errors); amp off:
    relative max error <= 1e-4.
  * no library GEMM or attention in a tower of two blocks (one windowed, one full) and the merger at the 7B widths.
"""
import json
import os
import traceback

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import golden_io
import qwen_case as qc
from conftest import ROOT
from det_init import det_init

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "qwen_golden.npz")
HEADS, HD = 2, 80
WIN140, WIN168 = [64, 16, 16, 4] * 2, [64, 32, 32, 16] * 2
SEGMENT_SETS = {"win140": WIN140, "win168": WIN168, "full100": [100, 100], "full324": [324, 324], "single4": [4]}


def _tables(T, g):
    ang = torch.rand(T, HD // 2, generator=g) * 40.0
    emb = torch.cat((ang, ang), -1)
    return emb.cos().contiguous(), emb.sin().contiguous()


def _rot(x):
    return torch.cat((-x[..., HD // 2:], x[..., :HD // 2]), -1)


def _attention_ref(qkv, cos, sin, lengths):
    """fp64, per segment; the rotated q and k rounded to bf16 first. qkv bf16 [T, 3 H d] on the CPU."""
    T = qkv.shape[0]
    q, k, v = qkv.double().reshape(T, 3, HEADS, HD).unbind(1)
    c, s = cos.double()[:, None], sin.double()[:, None]
    q = (q * c + _rot(q) * s).to(torch.bfloat16).double()
    k = (k * c + _rot(k) * s).to(torch.bfloat16).double()
    out = torch.empty(T, HEADS, HD, dtype=torch.float64)
    pos = 0
    for n in lengths:
        sl = slice(pos, pos + n)
        sc = torch.einsum("qhd,khd->hqk", q[sl], k[sl]) * HD ** -0.5
        out[sl] = torch.einsum("hqk,khd->qhd", sc.softmax(-1), v[sl])
        pos += n
    return out.reshape(T, HEADS * HD)


def _segments(lengths):
    from torch_utils.ops import vit_ops
    return vit_ops.Segments(lengths, DEV)


def _run_attention(qkv, cos, sin, seg, hint):
    from torch_utils.ops import qwen_hip
    out = torch.full((qkv.shape[0], HEADS * HD), float("nan"), dtype=torch.bfloat16, device=DEV)   # poison
    qwen_hip.rope_attention_varlen(qkv, cos, sin, seg.cu, HEADS, hint, out=out)
    return out


@pytest.mark.parametrize("mode", ["auto", "waves1", "waves4", "waves8"])
@pytest.mark.parametrize("name", list(SEGMENT_SETS))
def test_varlen_rope_attention(name, mode, monkeypatch):
    """'auto': the library's workgroup choice from the longest segment (2 waves for segments <= 64 keys, 4 up to 511,
    8 beyond: the tower test below runs that one at 1024);
    'waves4': the 4-wave kernel on every set, where waves skip the key tiles outside their own queries' segments;
    'waves1' / 'waves8': the 1-wave and 8-wave (256-query) A/B forms."""
    from torch_utils.ops import kernel_timer
    if mode in ("waves1", "waves8"):
        monkeypatch.setenv("VFM_QWEN_ATTN_WAVES", mode[-1])
    hint = "unknown" if mode == "waves4" else "max"
    lengths = SEGMENT_SETS[name]
    T = sum(lengths)
    g = torch.Generator().manual_seed(T + len(lengths))
    qkv = torch.randn(T, 3 * HEADS * HD, generator=g).to(torch.bfloat16)
    cos, sin = _tables(T, g)
    seg = _segments(lengths)
    kernel_timer.enable(True)
    out = _run_attention(qkv.to(DEV), cos.to(DEV), sin.to(DEV), seg, seg.max_len if hint == "max" else 0)
    torch.cuda.synchronize()
    waves = {"auto": 2 if max(lengths) <= 64 else 4, "waves1": 1, "waves4": 4, "waves8": 8}[mode]
    assert f"rope_attention_varlen<bf16,80,{waves}>" in kernel_timer.summary()
    kernel_timer.enable(False)
    out = out.cpu()
    assert not torch.isnan(out.float()).any(), "output elements left unwritten"
    ref = _attention_ref(qkv, cos, sin, lengths)
    err = (out.double() - ref).abs()
    m = float(ref.abs().max())
    print(f"{name} {mode}: max {float(err.max()) / m:.2e} mean {float(err.mean()) / m:.2e} of max|ref|")
    assert float(err.max()) <= 1.5e-2 * m, (float(err.max()), m)
    assert float(err.mean()) <= 2e-3 * m, (float(err.mean()), m)


@pytest.mark.parametrize("name,which", [("win140", 0), ("win140", 3), ("win140", 5), ("win168", 2), ("full324", 1),
                                         ("full100", 0)])
def test_varlen_attention_no_key_leaks(name, which):
    lengths = SEGMENT_SETS[name]
    T = sum(lengths)
    g = torch.Generator().manual_seed(T + which)
    qkv = torch.randn(T, 3, HEADS * HD, generator=g).to(torch.bfloat16)
    cos, sin = _tables(T, g)
    seg = _segments(lengths)
    start = sum(lengths[:which])
    sl = slice(start, start + lengths[which])
    other = qkv.clone()
    fresh = (torch.randn(T, 2, HEADS * HD, generator=g) * 3).to(torch.bfloat16)
    keep = other[sl].clone()
    other[:, 1:] = fresh                      # every K and V ...
    other[sl] = keep                          # ... except this segment's
    for hint in (seg.max_len, 0):
        a = _run_attention(qkv.reshape(T, -1).to(DEV), cos.to(DEV), sin.to(DEV), seg, hint)
        b = _run_attention(other.reshape(T, -1).to(DEV), cos.to(DEV), sin.to(DEV), seg, hint)
        assert torch.equal(a[sl].view(torch.int16), b[sl].view(torch.int16)), (name, which, hint)
        assert not torch.equal(a.view(torch.int16), b.view(torch.int16))       # the other segments did change


def test_other_head_dims_take_the_fallback():
    from torch_utils import custom_ops
    from torch_utils.ops import vit_ops
    lib = custom_ops.get_native()
    T, d = 40, 64
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(T, 3 * HEADS * d, generator=g).to(torch.bfloat16).to(DEV)
    ang = torch.rand(T, d // 2, generator=g)
    cos, sin = torch.cat((ang, ang), -1).cos().to(DEV), torch.cat((ang, ang), -1).sin().to(DEV)
    seg = _segments([24, 16])
    out = torch.empty(T, HEADS * d, dtype=torch.bfloat16, device=DEV)
    rc = lib.vfm_rope_attention_varlen(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), seg.cu.data_ptr(),
                                       out.data_ptr(), T, HEADS, d, 2, d ** -0.5, 0, custom_ops.stream_ptr(DEV))
    assert rc == custom_ops.VFM_NO_KERNEL
    got = vit_ops.rope_attention_varlen(qkv, cos, sin, seg, HEADS)
    want = vit_ops.rope_attention_varlen(qkv.cpu(), cos.cpu(), sin.cpu(), seg, HEADS)
    assert (got.cpu().float() - want.float()).abs().max() <= 2e-2 * want.float().abs().max()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("D", [320, 1280])
def test_rms_norm_rows(D, dtype):
    from torch_utils.ops import qwen_hip
    rows, eps = 67, 1e-6
    g = torch.Generator().manual_seed(D)
    h = (torch.randn(rows, D, generator=g) * 2).to(dtype)
    delta = torch.randn(rows, D, generator=g).to(dtype)
    w = 1.0 + 0.3 * torch.randn(D, generator=g)
    rel, floor = (2.0 ** -7, 1e-12) if dtype == torch.bfloat16 else (1e-5, 1e-12)

    def ref(x):
        x = x.double()
        return w.double() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))

    _, y = qwen_hip.rms_norm(h.to(DEV), None, w.to(DEV), eps)
    r = ref(h)
    assert y.dtype == dtype and ((y.cpu().double() - r).abs() <= rel * r.abs() + floor).all()
    # fused: h_out = round(h + delta) exactly, and the norm reads that rounded sum
    h_out, y = qwen_hip.rms_norm(h.to(DEV), delta.to(DEV), w.to(DEV), eps)
    want = (h.float() + delta.float()).to(dtype)
    assert torch.equal(h_out.cpu(), want)
    r = ref(want)
    assert ((y.cpu().double() - r).abs() <= rel * r.abs() + floor).all()
    h_only, none = qwen_hip.rms_norm(h.to(DEV), delta.to(DEV), None, eps, want_y=False)
    assert none is None and torch.equal(h_only.cpu(), want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("inter", [172, 3420])
def test_swiglu_rows(inter, dtype):
    from torch_utils.ops import qwen_hip
    rows, Ip = 37, (inter + 63) // 64 * 64
    g = torch.Generator().manual_seed(inter)
    gu = (torch.randn(rows, 2 * Ip, generator=g) * 2).to(dtype)       # the pad columns hold values too
    out = qwen_hip.swiglu(gu.to(DEV), inter).cpu()
    assert out.shape == (rows, Ip) and out.dtype == dtype
    assert not out[:, inter:].any(), "pad columns must be exactly zero"
    gd, ud = gu[:, :inter].double(), gu[:, Ip:Ip + inter].double()
    r = (gd * torch.sigmoid(gd)).to(dtype).double() * ud
    rel = 2.0 ** -6 if dtype == torch.bfloat16 else 1e-5
    assert ((out[:, :inter].double() - r).abs() <= rel * r.abs() + 1e-12).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_patch_gather_bitwise(dtype):
    from networks.utils.vfms.qwen_utils import window_layout
    from torch_utils.ops import vit_ops
    img = torch.randn(2, 3, 140, 140, generator=torch.Generator().manual_seed(2))
    idx = window_layout(2, 10, 10)[0].to(torch.int32)
    got = vit_ops.patch_rows(img.to(DEV), idx.to(DEV), 14, 640, dtype).cpu()
    want = vit_ops.patch_rows(img, idx, 14, 640, dtype)                 # the torch permutation (CPU path)
    assert got.shape == (200, 640) and got.dtype == dtype
    assert torch.equal(got, want) and not got[:, 588:].any()


# ------------------------------------------------------------------ the tower

@pytest.fixture(scope="module")
def golden():
    z = golden_io.load_npz(GOLDEN)
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def encoder_gpu(tmp_path_factory):
    from networks.utils.vfms.qwen_utils import QwenVisionEncoder
    d = tmp_path_factory.mktemp("qwen") / qc.VFM_DIRNAME
    d.mkdir()
    json.dump(dict(vision_config=qc.VISION_CFG), open(d / "config.json", "w"))
    enc = QwenVisionEncoder(model_name=str(d), scale_factor=1.0, patch_from_layers=list(qc.LAYERS), amp_enabled=False)
    det_init(enc.vision_model)
    return enc.eval().to(DEV)


def _relmax(a, b):
    a, b = a.double().cpu(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


def _rel_l2(a, b):
    a, b = a.double().cpu(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", qc.CASES, ids=[c["name"] for c in qc.CASES])
def test_tower_matches_reference_gpu(encoder_gpu, golden, case, precision):
    z, meta = golden
    name = case["name"]
    img = qc.image(case["res"], case["seed"])
    assert abs(float(img.double().sum()) - meta[f"{name}/img_sum"]) < 1e-6
    encoder_gpu.amp_enabled = precision == "bf16"
    try:
        feats, pooled = encoder_gpu.encode_image(img.to(DEV), case["eq_scale"], case["prior"])
    finally:
        encoder_gpu.amp_enabled = False
    stride = meta["row_stride"]
    report, failed = {}, []
    for hname, f in zip(qc.HIDDEN_NAMES, feats):
        assert list(f.shape) == meta[f"{name}/{hname}/shape"] and f.dtype == torch.float32
        rows = f if hname == "merged" else f[:, ::stride]
        if precision == "fp32":
            e, bound = _relmax(rows, z[f"{name}/{hname}/rows"]), 1e-4
        else:
            e, bound = _rel_l2(rows, z[f"{name}/{hname}/rows"]), 2 * meta[f"{name}/{hname}/e_bf16"]
        report[hname] = (e, bound)
        if e > bound:
            failed.append(hname)
    ref_pooled = z[f"{name}/pooled"]
    ep = _relmax(pooled, ref_pooled) if precision == "fp32" else _rel_l2(pooled, ref_pooled)
    report["pooled"] = (ep, 1e-4 if precision == "fp32" else 2 * meta[f"{name}/e_bf16"])
    print(f"{precision} {name}: " + ", ".join(f"{k} {e:.2e} (<= {b:.2e})" for k, (e, b) in report.items()))
    assert pooled.dtype == torch.float32 and not failed and ep <= report["pooled"][1], report


LIB_OPS = ("aten.mm", "aten.bmm", "aten.addmm", "aten.baddbmm", "aten.addbmm", "aten.matmul", "aten.linear",
           "aten.convolution", "aten._convolution", "aten.cudnn_convolution", "aten.miopen_convolution",
           "aten.convolution_backward", "aten._scaled_dot_product", "aten.addmv", "aten.mv", "aten.dot")


class _Record(TorchDispatchMode):
    """tests/test_no_vendor_gemm_gpu.py's recorder: every aten matrix product / convolution / fused attention on a
    ROCm tensor (where hipBLASLt, MIOpen or the library attention would run)."""

    def __init__(self):
        super().__init__()
        self.hits = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if name.startswith(LIB_OPS) and any(isinstance(a, torch.Tensor) and a.is_cuda for a in args):
            where = [f"{os.path.relpath(f.filename, ROOT)}:{f.lineno}" for f in traceback.extract_stack()
                     if ROOT in f.filename and "tests" not in f.filename][-3:]
            shapes = [tuple(a.shape) for a in args if isinstance(a, torch.Tensor)]
            self.hits.append((name, shapes, " < ".join(where)))
        return func(*args, **(kwargs or {}))


def test_tower_runs_no_library_gemm_or_attention(tmp_path):
    """Two blocks (one windowed, one full) and the merger at the 7B widths, B = 2 at 448^2, bf16."""
    from networks.utils.vfms.qwen_utils import QwenVisionEncoder
    from torch_utils.ops import kernel_timer
    d = tmp_path / "qwen2.5-vl-two-blocks"
    d.mkdir()
    json.dump(dict(vision_config=dict(depth=2, hidden_size=1280, num_heads=16, intermediate_size=3420,
                                      out_hidden_size=3584, fullatt_block_indexes=[1], window_size=112)),
              open(d / "config.json", "w"))
    enc = QwenVisionEncoder(model_name=str(d), scale_factor=1.0, patch_from_layers=[0, 1, -1]).eval().to(DEV)
    img = torch.rand(2, 3, 448, 448, generator=torch.Generator().manual_seed(0)).to(DEV)
    enc.encode_image(img)                          # warm: weight casts and padded copies are cached
    kernel_timer.enable(True)
    rec = _Record()
    with rec:
        feats, pooled = enc.encode_image(img)
    torch.cuda.synchronize()
    seen = list(kernel_timer.summary())
    kernel_timer.enable(False)
    assert [tuple(f.shape) for f in feats] == [(2, 1024, 1280), (2, 1024, 1280), (2, 256, 3584)]
    assert all(torch.isfinite(f).all() for f in feats) and torch.isfinite(pooled).all()
    msg = "\n".join(f"{h[0]} {h[1]} {h[2]}" for h in rec.hits)
    assert not rec.hits, f"library GEMM / attention calls in the tower:\n{msg}"
    assert "rope_attention_varlen<bf16,80,2>" in seen and "rope_attention_varlen<bf16,80,8>" in seen, seen
    assert any(k.startswith("gemm9<bf16") for k in seen), seen
