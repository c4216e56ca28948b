"""SigLIP2 text conditioning on cuda:0 against the reference's golden vectors (tests/golden/make_golden_text.py).

  * the text tower under bf16: `seq_tokens` and `pooled` within 2 x the stored e_bf16 (relative L2; two independent
    bf16 evaluations of one fp32 function can differ by the sum of their errors, tests/test_qwen_gpu.py), masks exact,
    the key-masked attention kernel on record; fp32 (amp off): relative L2 <= 1e-4;
  * no library GEMM or attention in the tower (tests/test_qwen_gpu.py's recorder), at the SigLIP2-base widths;
  * the text-conditional Generator against the stored fixture, every stored element, with tests/test_networks_gpu.py's
    bounds (fp32: 1e-4 / 2e-3 / 1e-3; bf16 decoder blocks and towers: 3e-2 / 1e-1 / 5e-2; the latent's gradient in
    bf16: 2 x the fixture's e_bf16_max = 1.47e-1, measured 1.09e-1), the cross-attention kernels on record.
"""
import json

import numpy as np
import pytest
import torch

import text_case as tc
from det_init import det_init
from test_networks_gpu import TOL
from test_qwen_gpu import _Record
from test_text import _arr, _meta, _rel_l2, check_generator

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def vfm_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("vfm_text_gpu") / tc.VFM_DIRNAME
    d.mkdir()
    json.dump(tc.config_json(), open(d / "config.json", "w"))
    return str(d)


@pytest.fixture(scope="module")
def encoder_gpu(vfm_dir):
    from networks.utils.vfms.siglip2_utils import SigLIP2Encoder
    enc = SigLIP2Encoder(model_name=vfm_dir, conditional=True, label_type="cls2text", scale_factor=1.0,
                         patch_from_layers=[0, 1, -1], amp_enabled=False)
    det_init(enc.text_model, prefix="text_model.")
    return enc.eval().to(DEV)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_text_tower_matches_reference_gpu(encoder_gpu, precision):
    from torch_utils.ops import kernel_timer
    encoder_gpu.amp_enabled = precision == "bf16"
    kernel_timer.enable(True)
    try:
        seq, pooled, mask = encoder_gpu.encode_text(list(tc.STRINGS))
        torch.cuda.synchronize()
        seen = list(kernel_timer.summary())
    finally:
        kernel_timer.enable(False)
        encoder_gpu.amp_enabled = False
    assert seq.dtype == pooled.dtype == torch.float32 and mask.dtype == torch.bool and seq.is_cuda
    assert np.array_equal(mask.cpu().numpy(), _arr("mask").astype(bool))
    meta = _meta()
    report = {}
    for name, got in zip(tc.TOKENS, (seq, pooled)):
        bound = 2 * meta[f"{name}/e_bf16"] if precision == "bf16" else 1e-4
        report[name] = (_rel_l2(got.cpu(), _arr(name)), bound)
    print(f"{precision}: " + ", ".join(f"{k} {e:.2e} (<= {b:.2e})" for k, (e, b) in report.items()))
    assert all(e <= b for e, b in report.values()), report
    if precision == "bf16":
        assert "attention_keymask_fwd<bf16,64>" in seen, seen


def test_text_tower_runs_no_library_gemm_or_attention(tmp_path):
    """Two layers at the SigLIP2-base text widths (768, 12 heads of 64, 3072), B = 8, bf16."""
    from networks.utils.vfms.siglip2_utils import SigLIP2Encoder
    from torch_utils.ops import kernel_timer
    d = tmp_path / "siglip2-base-two-layers"
    d.mkdir()
    text = dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=2, intermediate_size=3072, vocab_size=300,
                max_position_embeddings=64)
    json.dump(dict(text_config=text, vision_config=tc.VISION_CFG), open(d / "config.json", "w"))
    enc = SigLIP2Encoder(model_name=str(d), conditional=True, label_type="text", scale_factor=1.0,
                         patch_from_layers=[-1]).eval().to(DEV)
    texts = ["", "tabby!", "a photo of a cat", tc.STRINGS[2]] * 2
    enc.encode_text(texts)                         # warm: weight casts are cached
    kernel_timer.enable(True)
    rec = _Record()
    with rec:
        seq, pooled, mask = enc.encode_text(texts)
    torch.cuda.synchronize()
    seen = list(kernel_timer.summary())
    kernel_timer.enable(False)
    assert seq.shape == (8, 64, 768) and pooled.shape == (8, 768) and mask.sum(1).tolist() == [1, 7, 17, 64] * 2
    assert torch.isfinite(seq).all() and torch.isfinite(pooled).all()
    msg = "\n".join(f"{h[0]} {h[1]} {h[2]}" for h in rec.hits)
    assert not rec.hits, f"library GEMM / attention calls in the text tower:\n{msg}"
    assert "attention_keymask_fwd<bf16,64>" in seen and any(k.startswith("gemm9<bf16") for k in seen), seen


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_conditional_generator_gpu(vfm_dir, precision):
    from networks.generator import Generator
    from torch_utils.ops import kernel_timer
    over = {} if precision == "bf16" else dict(num_fp16_res=0)
    torch.manual_seed(0)
    G = Generator(label_dim=0, **dict(tc.g_kwargs(vfm_dir), **over)).train()
    det_init(G)
    G = G.to(DEV)
    G.vfm_encoder.encoder.amp_enabled = precision == "bf16"
    img = tc.image().to(DEV)
    with torch.no_grad():                           # first forward: records the grouped style plan
        G(img, list(tc.STRINGS), validation=True)
    kernel_timer.enable(True)
    try:
        res = tc.run_generator(G, img, tc.STRINGS)
        torch.cuda.synchronize()
        seen = {k.split("<")[0] for k in kernel_timer.summary()}
    finally:
        kernel_timer.enable(False)
    assert {"cross_attention_fwd", "cross_attention_bwd"} <= seen, sorted(seen)
    tol = TOL[precision]
    # Every stored element is held. tests/test_networks_gpu.py's `full` bound is one for parameter gradients (to_q,
    # to_kv, null_kv); it has none for an activation gradient. In bf16 the latent's gradient is held to twice the
    # reference's own bf16 error of that tensor in the same metric (the fixture's e_bf16_max: the reference
    # generator under bf16 autocast against its fp32 result), the project's bound for two independent bf16
    # evaluations of one fp32 function; in fp32 to `full` like the others.
    tols = {"grad/z": 2 * _meta()["G/grad/z/e_bf16_max"]} if precision == "bf16" else None
    check_generator(res, f"gpu {precision}", out_tol=tol["out"], full_tol=tol["full"], norm_tol=tol["norm"], tols=tols)
