"""Qwen2.5-VL vision tower (networks/utils/vfms/qwen_utils.py), CPU side: the torch formulation (which is also
what the kernels fall back to) against vectors generated from the reference itself
(tests/golden/make_golden_qwen.py) and against the HF transformers model directly, fp32: relative max error
<= 1e-4, the project's bound for fp32 towers (different GEMM / attention kernels, the folded temporal weight
slices). Plus the interface: output shapes and token order, `token_strides`, the Generator on the merged grid,
loading with either checkpoint key prefix, the text path."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import golden_io
import qwen_case as qc
from det_init import det_init

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "qwen_golden.npz")
MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 3, 1, 1)
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 3, 1, 1)


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope="module")
def golden():
    z = golden_io.load_npz(GOLDEN)
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def config_dir(tmp_path_factory):
    """A local directory with only a config.json (nested vision_config, as HF saves it)."""
    d = tmp_path_factory.mktemp("qwen") / qc.VFM_DIRNAME
    d.mkdir()
    json.dump(dict(vision_config=qc.VISION_CFG, text_config=qc.TEXT_CFG), open(d / "config.json", "w"))
    return str(d)


@pytest.fixture(scope="module")
def encoder(config_dir):
    from networks.utils.vfms.qwen_utils import QwenVisionEncoder
    enc = QwenVisionEncoder(model_name=config_dir, scale_factor=1.0, patch_from_layers=list(qc.LAYERS),
                            amp_enabled=False)
    assert not enc.pretrained_loaded
    det_init(enc.vision_model)
    return enc.eval()


@pytest.mark.parametrize("case", qc.CASES, ids=[c["name"] for c in qc.CASES])
def test_matches_reference_golden_cpu(encoder, golden, case):
    z, meta = golden
    name = case["name"]
    img = qc.image(case["res"], case["seed"])
    assert abs(float(img.double().sum()) - meta[f"{name}/img_sum"]) < 1e-6
    feats, pooled = encoder.encode_image(img, case["eq_scale"], case["prior"])
    stride = meta["row_stride"]
    for hname, f in zip(qc.HIDDEN_NAMES, feats):
        assert list(f.shape) == meta[f"{name}/{hname}/shape"], (name, hname, tuple(f.shape))
        assert f.dtype == torch.float32
        if hname == "merged":
            e = _rel(f, z[f"{name}/{hname}/rows"])
        else:
            e = max(_rel(f[:, ::stride], z[f"{name}/{hname}/rows"]),
                    _rel(f.double().norm(dim=-1), z[f"{name}/{hname}/norms"]))
        print(f"{name} {hname}: {e:.2e}")
        assert e <= 1e-4, (name, hname, e)
    assert pooled.dtype == torch.float32 and _rel(pooled, z[f"{name}/pooled"]) <= 1e-4


@pytest.mark.parametrize("case", qc.CASES, ids=[c["name"] for c in qc.CASES])
def test_window_layout_matches_hf(case):
    """The one-gather token order and the window lengths against HF's get_vision_window_index."""
    from transformers.vision_utils import get_vision_window_index
    from networks.utils.vfms.qwen_utils import window_layout
    grid = int(case["res"] * case["eq_scale"]) // 14
    w2r, u_w2r, lengths, py, px = window_layout(qc.BATCH, grid, grid)
    assert lengths == case["windows"] * qc.BATCH
    idx, cu = get_vision_window_index(torch.tensor([[1, grid, grid]] * qc.BATCH), spatial_merge_size=2,
                                      window_size=112, patch_size=14)
    assert torch.equal(u_w2r, idx)
    assert (cu[1:] - cu[:-1]).tolist() == lengths
    assert torch.equal(w2r.sort().values, torch.arange(qc.BATCH * grid * grid))
    assert torch.equal(w2r % (grid * grid), py * grid + px)


@pytest.fixture(scope="module")
def hf_dir(tmp_path_factory):
    from transformers import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration
    d = str(tmp_path_factory.mktemp("m") / "tiny-qwen2.5-vl-hf")
    torch.manual_seed(0)
    m = Qwen2_5_VLForConditionalGeneration(Qwen2_5_VLConfig(vision_config=dict(qc.VISION_CFG),
                                                            text_config=dict(qc.TEXT_CFG))).float()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "visual" in n:
                p.add_(torch.randn_like(p) * 0.05)      # biases and norm weights away from their 0 / 1 init
    m.save_pretrained(d)
    return d


def _hf_forward(hf_dir, img):
    """The reference wrapper's patchify (qwen_utils.py:154-199) and the HF vision model."""
    from transformers import Qwen2_5_VLForConditionalGeneration
    full = Qwen2_5_VLForConditionalGeneration.from_pretrained(hf_dir).float().eval()
    visual = full.model.visual if hasattr(full.model, "visual") else full.visual
    x = (img - MEAN) / STD
    B, C, H, W = x.shape
    gh, gw = H // 14, W // 14
    x = x.unsqueeze(1).repeat(1, 2, 1, 1, 1)
    x = x.reshape(B, 1, 2, C, gh // 2, 2, 14, gw // 2, 2, 14).permute(0, 1, 4, 7, 5, 8, 3, 2, 6, 9)
    flat = x.reshape(B, gh * gw, C * 2 * 14 * 14)
    with torch.no_grad():
        out = visual(flat, grid_thw=torch.tensor([[1, gh, gw]] * B))
    out = out if isinstance(out, torch.Tensor) else out.pooler_output
    return out.reshape(B, -1, out.shape[-1])


@pytest.mark.parametrize("size", [140, 196])
def test_matches_hf(hf_dir, size):
    from networks.utils.vfms.qwen_utils import QwenVisionEncoder
    enc = QwenVisionEncoder(model_name=hf_dir, scale_factor=1.0, patch_from_layers=[-1])
    assert enc.pretrained_loaded
    img = torch.rand(2, 3, size, size, generator=torch.Generator().manual_seed(5))
    feats, pooled = enc.encode_image(img, 1.0, False)
    ref = _hf_forward(hf_dir, img)
    assert feats[0].shape == ref.shape == (2, (size // 28) ** 2, 128)
    assert _rel(feats[0], ref) <= 1e-4
    assert _rel(pooled, ref.mean(1)) <= 1e-4


def test_shapes_and_raster_order(encoder):
    """Index 0, a block index and -1: [B, gh gw, D] / [B, gh gw / 4, out], index 0 in raster order of the grid."""
    img = qc.image(168, 7)
    feats, pooled = encoder.encode_image(img)
    assert [tuple(f.shape) for f in feats] == [(2, 144, 320), (2, 144, 320), (2, 36, 128)]
    assert pooled.shape == (2, 128)
    assert _rel(pooled, feats[2].mean(1)) <= 1e-6
    w = encoder.vision_model.patch_embed.proj.weight.sum(2)                 # both temporal slices see the frame
    direct = F.conv2d((img - MEAN) / STD, w, stride=14).flatten(2).transpose(1, 2)
    assert _rel(feats[0], direct) <= 1e-4
    # negative block indices count from the last block: -2 = block 4, -4 = block 2
    from networks.utils.vfms.qwen_utils import QwenVisionEncoder
    enc2 = QwenVisionEncoder(model_name=encoder.model_name, patch_from_layers=[-4, -2], amp_enabled=False)
    det_init(enc2.vision_model)
    f2, _ = enc2.encode_image(img)
    assert torch.equal(f2[0], feats[1]) and f2[1].shape == (2, 144, 320) and not torch.equal(f2[1], f2[0])
    with pytest.raises(ValueError):
        QwenVisionEncoder(model_name=encoder.model_name, patch_from_layers=[5])


def test_padding_changes_nothing(encoder):
    """The zero-padded GEMM operands (intermediate 172 -> 192, patch K 588 -> 640) against the unpadded products."""
    blk = encoder.vision_model.blocks[0].mlp
    n = torch.randn(10, 320, generator=torch.Generator().manual_seed(3))
    ref = blk.down_proj(F.silu(blk.gate_proj(n)) * blk.up_proj(n))
    w, b, wd = blk._padded(torch.float32)
    assert w.shape == (384, 320) and wd.shape == (320, 192)
    assert not w[172:192].any() and not w[364:].any() and not b[172:192].any() and not wd[:, 172:].any()
    assert _rel(blk(n), ref) <= 1e-5
    assert encoder.vision_model.patch_weight(torch.float32).shape == (320, 640)


def test_token_strides(config_dir):
    from networks.utils.vfm_utils import VFMEncoder
    enc = VFMEncoder(config_dir, False, "cls2text", 1.0, [0, 2, -1])
    assert enc.patch_size == 14
    assert enc.token_strides == [14, 14, 28]
    assert enc.encoder.token_strides == [14, 14, 28]


def test_token_strides_absent_on_other_backbones(tmp_path):
    from transformers import Dinov2Config
    from networks.utils.vfm_utils import VFMEncoder
    d = tmp_path / "tiny-dinov2-local"
    d.mkdir()
    json.dump(Dinov2Config(hidden_size=64, num_hidden_layers=1, num_attention_heads=4, image_size=56,
                           patch_size=14).to_dict(), open(d / "config.json", "w"))
    assert VFMEncoder(str(d), False, "cls2text", 1.0, [-1]).token_strides is None


@torch.no_grad()
def test_generator_encodes_on_the_merged_grid(config_dir):
    """The synthetic stage-0 YAML with the tiny tower: 256^2, scale 1.75 -> 448^2 -> 32 x 32 patches -> 16 x 16
    merged tokens, which the adapter takes at down-scale factor 1 (z is 16 x 16)."""
    import yaml
    import dnnlib
    from conftest import PKG
    from train import resolve_config
    raw = yaml.safe_load(open(os.path.join(PKG, "configs", "vfm_vae_f16d32_qwen2_5_vl_stage_0_synthetic.yaml")))
    assert raw["G_kwargs"]["scale_factor"] == 1.75 and raw["G_kwargs"]["patch_from_layers"] == [-1]
    assert "qwen" in raw["G_kwargs"]["vfm_name"].lower() and raw["G_kwargs"]["patch_in_dimensions"] == [3584]
    raw["G_kwargs"].update(vfm_name=config_dir, patch_in_dimensions=[128])
    c = resolve_config(raw)
    torch.manual_seed(0)
    G = dnnlib.util.construct_class_by_name(label_dim=0, **c.G_kwargs).eval()
    assert G.patch_resolutions == [16]
    img = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(1))
    feats, pooled = G.vfm_encoder.encode_image(img)
    assert feats[0].shape == (1, 256, 128)
    z = G.encode(img)
    assert z.shape == (1, 32, 16, 16) and torch.isfinite(z).all()


@pytest.mark.parametrize("prefix", ["visual.", "model.visual."])
def test_loads_both_key_prefixes(encoder, config_dir, tmp_path, prefix):
    """A checkpoint with either prefix of the vision keys (transformers 4.50 / 5.x) plus language-model tensors."""
    import shutil
    from safetensors.torch import save_file
    from networks.utils.vfms.qwen_utils import QwenVisionEncoder
    d = tmp_path / "qwen-ckpt"
    d.mkdir()
    shutil.copy(os.path.join(config_dir, "config.json"), d / "config.json")
    state = {prefix + k: v.clone() for k, v in encoder.vision_model.state_dict().items()}
    state["model.language_model.layers.0.mlp.up_proj.weight"] = torch.zeros(4, 4)
    state["lm_head.weight"] = torch.zeros(4, 4)
    save_file(state, str(d / "model.safetensors"))
    enc = QwenVisionEncoder(model_name=str(d), patch_from_layers=list(qc.LAYERS), amp_enabled=False)
    assert enc.pretrained_loaded
    for k, v in encoder.vision_model.state_dict().items():
        assert torch.equal(enc.vision_model.state_dict()[k], v), k
    # a checkpoint that lacks a vision tensor is an error, not a silent random init
    del state[prefix + "merger.mlp.2.bias"]
    save_file(state, str(d / "model.safetensors"))
    with pytest.raises(RuntimeError):
        QwenVisionEncoder(model_name=str(d), patch_from_layers=[-1])


def test_text_path_raises(config_dir):
    from networks.utils.vfm_utils import VFMEncoder
    for label_type in ("text", "cls2text"):
        with pytest.raises(NotImplementedError):
            VFMEncoder(config_dir, True, label_type, 1.0, [-1])
    assert VFMEncoder(config_dir, False, "cls2text", 1.0, [-1]).encode_text(["a"]) == (None, None, None)


def test_default_dimensions_are_the_7b_tower():
    from networks.utils.vfms.qwen_utils import qwen_config_from_name
    cfg = qwen_config_from_name("Qwen/Qwen2.5-VL-7B-Instruct")
    assert (cfg["depth"], cfg["hidden_size"], cfg["num_heads"], cfg["intermediate_size"], cfg["out_hidden_size"],
            cfg["window_size"], cfg["fullatt_block_indexes"]) == (32, 1280, 16, 3420, 3584, 112, [7, 15, 23, 31])
