"""SigLIP2 text conditioning on the CPU, fp32, against the reference's golden vectors
(tests/golden/make_golden_text.py; tests/text_case.py is the shared tiny configuration).

  * the conditional encoder can be constructed (it raised NotImplementedError before the text tower existed) and
    `encode_text` reproduces the reference's masks exactly and its `seq_tokens` / `pooled` to relative L2 <= 1e-4
    (the fp32 bound of tests/test_qwen_gpu.py's pooled output);
  * checkpoint loading takes the `text_model.` prefix and the flat names; the tokenizer rule;
  * the unconditional encoder is unchanged;
  * the text-conditional Generator reproduces gen_img / global_text_tokens (tests/test_networks_parity.py: 1e-4 of
    the maximum) and the stored gradients (its full_tol 2e-3 of the maximum, norms 1e-3);
  * the text-conditional YAML builds through the path tests/test_configs.py exercises.
"""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import golden_io
import text_case as tc
from conftest import PKG
from det_init import canonical, det_init
from test_networks_parity import _rel

GOLDEN = "text_golden.npz"


def _arr(k):
    return golden_io.load(GOLDEN)[0][k]


def _meta():
    return golden_io.load(GOLDEN)[1]


def _rel_l2(a, b):
    a, b = a.double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def vfm_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("vfm_text") / tc.VFM_DIRNAME
    d.mkdir()
    json.dump(tc.config_json(), open(d / "config.json", "w"))
    return str(d)


def _encoder(vfm_dir, **over):
    from networks.utils.vfms.siglip2_utils import SigLIP2Encoder
    kw = dict(model_name=vfm_dir, conditional=True, label_type="cls2text", scale_factor=1.0,
              patch_from_layers=[0, 1, -1], amp_enabled=False)
    kw.update(over)
    return SigLIP2Encoder(**kw)


@pytest.fixture(scope="module")
def encoder(vfm_dir):
    enc = _encoder(vfm_dir)
    det_init(enc.text_model, prefix="text_model.")
    return enc.eval()


def test_conditional_encoder_constructs(encoder):
    from networks.utils.vfms.siglip2_utils import ByteTokenizer
    tm = encoder.text_model
    assert tm.config.hidden_size == 128 and tm.config["projection_size"] == 128
    assert encoder.use_text and isinstance(encoder.tokenizer, ByteTokenizer)
    assert not any(p.requires_grad for p in tm.parameters()) and not tm.training
    assert sorted(tm.state_dict().keys()) == _meta()["text_state_keys"]       # the HF module tree
    assert tm.embeddings.position_embedding.num_embeddings == 64
    import copy
    twin = copy.deepcopy(encoder)                  # the training loop deep-copies the generator into its EMA twin
    assert twin.text_model.config.hidden_size == 128 and not hasattr(tm.config, "no_such_key")


def test_tokenizer_stand_in_matches_the_fixture(encoder):
    out = encoder.tokenizer(list(tc.STRINGS), padding="max_length", max_length=64, truncation=True, return_tensors="pt",
                            return_attention_mask=True)
    assert _meta()["strings"] == list(tc.STRINGS)
    assert np.array_equal(out["input_ids"].numpy(), _arr("ids"))
    assert np.array_equal(out["attention_mask"].numpy(), _arr("mask"))
    same = tc.ByteTokenizer()(list(tc.STRINGS))
    assert torch.equal(same["input_ids"], out["input_ids"]) and torch.equal(same["attention_mask"], out["attention_mask"])
    assert out["attention_mask"].sum(1).tolist() == [1, 7, 64]                 # EOS only; 6 bytes + EOS; truncated
    assert int(out["input_ids"][2, -1]) != 1                                    # truncation dropped the EOS


def test_encode_text_matches_reference(encoder):
    seq, pooled, mask = encoder.encode_text(list(tc.STRINGS))
    assert seq.dtype == pooled.dtype == torch.float32 and mask.dtype == torch.bool
    assert seq.shape == (3, 64, 128) and pooled.shape == (3, 128)
    assert np.array_equal(mask.numpy(), _arr("mask").astype(bool))
    e_seq, e_pool = _rel_l2(seq, _arr("seq_tokens")), _rel_l2(pooled, _arr("pooled"))
    print(f"seq_tokens {e_seq:.2e}, pooled {e_pool:.2e} (<= 1e-4)")
    assert e_seq <= 1e-4 and e_pool <= 1e-4


def test_dropping_the_mask_changes_the_output(encoder):
    """The mask is not decoration: without it the padded samples move (the full-length one does not)."""
    ids, mask = torch.from_numpy(_arr("ids")), torch.from_numpy(_arr("mask"))
    with_mask, _ = encoder.text_model(ids, mask, compute_dtype=torch.float32)
    without, _ = encoder.text_model(ids, None, compute_dtype=torch.float32)
    assert _rel_l2(without[:2], with_mask[:2]) > 0.1
    assert _rel_l2(without[2:], with_mask[2:]) < 1e-5


@pytest.mark.parametrize("prefix", ["text_model.", ""], ids=["prefixed", "flat"])
def test_checkpoint_layouts(encoder, tmp_path, prefix):
    from safetensors.torch import save_file
    from networks.utils.vfms.siglip2_utils import SiglipTextModel, siglip_text_config_from_name
    d = tmp_path / tc.VFM_DIRNAME
    d.mkdir()
    json.dump(tc.config_json(), open(d / "config.json", "w"))
    state = {prefix + k: v.contiguous() for k, v in encoder.text_model.state_dict().items()}
    save_file(state, str(d / "model.safetensors"))
    tm = SiglipTextModel(siglip_text_config_from_name(str(d)))
    assert tm.load_hf_checkpoint(str(d))
    for k, v in encoder.text_model.state_dict().items():
        assert torch.equal(tm.state_dict()[k], v), k
    tm.load_state_dict(state)                      # the same two layouts through load_state_dict itself
    # weights without tokenizer files: the stand-in would feed ids the weights were not trained on
    with pytest.raises(FileNotFoundError, match=tc.VFM_DIRNAME):
        from networks.utils.vfms.siglip2_utils import load_tokenizer
        load_tokenizer(str(d), pretrained=True)


def test_missing_text_weights_are_reported(tmp_path):
    from safetensors.torch import save_file
    from networks.utils.vfms.siglip2_utils import SiglipTextModel, siglip_text_config_from_name
    d = tmp_path / tc.VFM_DIRNAME
    d.mkdir()
    json.dump(tc.config_json(), open(d / "config.json", "w"))
    save_file({"text_model.head.bias": torch.zeros(128)}, str(d / "model.safetensors"))
    with pytest.raises(RuntimeError, match="missing"):
        SiglipTextModel(siglip_text_config_from_name(str(d))).load_hf_checkpoint(str(d))


def test_random_init_by_name_is_reproducible():
    from networks.utils.vfms.siglip2_utils import ByteTokenizer, SiglipTextModel, siglip_text_config_from_name
    cfg = siglip_text_config_from_name("google/siglip2-base-patch16-256")
    assert (cfg.hidden_size, cfg.num_attention_heads, cfg.vocab_size) == (768, 12, ByteTokenizer.vocab_size)
    cfg = dict(cfg, num_hidden_layers=1)
    a, b = SiglipTextModel(cfg), SiglipTextModel(cfg)
    a.reset_parameters()
    b.reset_parameters()
    for (k, x), y in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(x, y), k


def test_unconditional_encoder_is_unchanged(vfm_dir):
    enc = _encoder(vfm_dir, conditional=False)
    assert enc.text_model is None and enc.tokenizer is None and not enc.use_text
    assert enc.encode_text(["a photo"]) == (None, None, None)
    assert not any(k.startswith("text_model") for k in enc.state_dict())


def test_qwen_text_conditioning_stays_out_of_scope():
    from networks.utils.vfms.qwen_utils import QwenVisionEncoder
    with pytest.raises(NotImplementedError):
        QwenVisionEncoder(model_name="Qwen/Qwen2.5-VL-7B-Instruct", conditional=True, label_type="cls2text",
                          scale_factor=1.0, patch_from_layers=[-1])


@pytest.fixture(scope="module")
def generator(vfm_dir):
    from networks.generator import Generator
    torch.manual_seed(0)
    G = Generator(label_dim=0, **tc.g_kwargs(vfm_dir)).train()
    det_init(G)
    return G


def check_generator(res, where, out_tol=1e-4, full_tol=2e-3, norm_tol=1e-3, tols=None):
    """gen_img / global_text_tokens and every element of the stored gradients against the fixture, with
    tests/test_networks_parity.py's bounds (the defaults; the GPU test passes tests/test_networks_gpu.py's): outputs
    1e-4 of the maximum, gradient tensors 2e-3 of the maximum, gradient norms 1e-3. tols: {name: element-wise bound}
    for single tensors, in place of out_tol / full_tol."""
    meta = _meta()
    arrays = golden_io.load(GOLDEN)[0]
    report, bad = [], []
    for k, v in res.items():
        ref = tc.load_chunks(arrays, "G/" + k)
        got = v.detach().cpu()
        assert tuple(got.shape) == ref.shape, k
        if not np.any(ref):                                   # null_kv: masked out whenever a mask is given
            assert not got.any(), k
            continue
        tol = (tols or {}).get(k, full_tol if k.startswith("grad/") else out_tol)
        e = _rel(got, ref)
        report.append(f"{k.rsplit('.attn.', 1)[-1]} {e:.2e} (<= {tol:.2e})")
        if not e < tol:
            bad.append(k)
        if k.startswith("grad/"):
            nm = meta[f"G/{k}/norm"]
            assert abs(float(v.double().norm()) - nm) < norm_tol * nm, (k, float(v.double().norm()), nm)
    print(f"{where}: " + ", ".join(report))
    assert not bad, (bad, report)


def test_conditional_generator_matches_reference(generator):
    assert sorted(canonical(k) for k in generator.state_dict()) == sorted(canonical(k) for k in _meta()["G_state_keys"])
    assert tc.grad_param_names(generator) == _meta()["G_grad_names"]
    assert generator.c_dim == 128 and generator.w_dim == 512 + 128
    check_generator(tc.run_generator(generator, tc.image(), tc.STRINGS), "cpu")


@torch.no_grad()
def test_text_config_builds_and_conditions(monkeypatch):
    """configs/vfm_vae_f16d32_siglip2_stage_0_text_synthetic.yaml through train.resolve_config and
    construct_class_by_name (tests/test_configs.py's path). The towers are cut to one layer each: what is under
    test is the YAML's keys reaching a conditional, cross-attending Generator, not the towers' depth."""
    import dnnlib
    from networks.utils.vfms import siglip2_utils
    from train import resolve_config
    c = resolve_config(yaml.safe_load(open(os.path.join(PKG, "configs",
                                                        "vfm_vae_f16d32_siglip2_stage_0_text_synthetic.yaml"))))
    assert c.G_kwargs.conditional is True and c.G_kwargs.label_type == "cls2text" and c.G_kwargs.use_cross_attn is True
    vis, txt = siglip2_utils.siglip_config_from_name, siglip2_utils.siglip_text_config_from_name
    monkeypatch.setattr(siglip2_utils, "siglip_config_from_name", lambda n: dict(vis(n), num_hidden_layers=1))
    monkeypatch.setattr(siglip2_utils, "siglip_text_config_from_name",
                        lambda n: siglip2_utils._Config(txt(n), num_hidden_layers=1))
    kw = dict(c.G_kwargs, patch_from_layers=[0, 1, -1])
    torch.manual_seed(0)
    G = dnnlib.util.construct_class_by_name(label_dim=0, **kw).eval()
    assert G.c_dim == 1024 and any(".cross_attns." in n for n, _ in G.named_parameters())
    fine, glob, mask = G.vfm_encoder.encode_text(["a photo", ""])
    assert fine.shape == (2, 64, 1024) and glob.shape == (2, 1024) and mask.sum(1).tolist() == [8, 1]
