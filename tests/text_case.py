"""The tiny SigLIP text / vision pair and the text-conditional generator shared by tests/golden/make_golden_text.py
(reference side) and the text tests (this package).

Text tower: hidden 128, 2 heads of 64, 2 layers, intermediate 256, vocabulary 300, 64 positions, projection 128.
Vision tower: tests/net_cases.py's. Weights come from tests/det_init.py on both sides (keyed by state-dict name),
so the tests rebuild both towers from a config.json alone.

Both sides tokenize with the byte stand-in below (the package's own copy is networks.utils.vfms.siglip2_utils.
ByteTokenizer; the tests check that the two produce the same ids): ids = UTF-8 bytes + 2, then EOS = 1, padded
with 0 to 64, mask = 1 over bytes + EOS. Truncation cuts the id list, EOS included, at 64: a text of 64 bytes or
more keeps 64 byte ids, all valid, and no EOS -- the way HF truncation drops the tail of an over-long input.
"""
import torch

import net_cases

VFM_DIRNAME = "siglip2-tiny-text-patch16-64"
TEXT_CFG = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, vocab_size=300,
                max_position_embeddings=64, projection_size=128, layer_norm_eps=1e-6, pad_token_id=0, bos_token_id=2,
                eos_token_id=1)
VISION_CFG = dict(net_cases.SIGLIP_CFG, layer_norm_eps=1e-6)
TEXT_LENGTH = 64
# "" -> only EOS valid; a 6-byte word; 78 bytes -> truncated to 64 valid ids without EOS
STRINGS = ("", "tabby!", "a photograph of a tabby cat asleep on a windowsill in the late afternoon light")
TOKENS = ("seq_tokens", "pooled")


class ByteTokenizer:
    pad_token_id, eos_token_id = 0, 1

    def __call__(self, text, padding="max_length", max_length=TEXT_LENGTH, truncation=True, return_tensors="pt",
                 return_attention_mask=True):
        text = [text] if isinstance(text, str) else list(text)
        ids = torch.full((len(text), max_length), self.pad_token_id, dtype=torch.int64)
        mask = torch.zeros(len(text), max_length, dtype=torch.int64)
        for i, t in enumerate(text):
            seq = ([b + 2 for b in t.encode("utf-8")] + [self.eos_token_id])[:max_length]
            ids[i, :len(seq)] = torch.tensor(seq, dtype=torch.int64)
            mask[i, :len(seq)] = 1
        return {"input_ids": ids, "attention_mask": mask}


def config_json():
    """config.json of the model directory: a full SigLIP config with both sub-configs."""
    return dict(model_type="siglip", text_config=dict(TEXT_CFG), vision_config=dict(VISION_CFG))


def g_kwargs(vfm_dir):
    return net_cases.g_kwargs(vfm_dir, conditional=True, label_type="cls2text", use_cross_attn=True)


def image(batch=len(STRINGS)):
    return torch.rand(batch, 3, 64, 64, generator=torch.Generator().manual_seed(17))


def loss_weights(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(18))


CHUNK_ELEMS = 131072     # one stored array stays under golden_io's part budget (incompressible fp32: 512 KiB)


def row_chunks(t):
    """A tensor as the fixture stores it: whole, in row blocks of at most CHUNK_ELEMS entries (key `<name>#<i>`)."""
    rows = max(1, CHUNK_ELEMS // max(1, t[0].numel())) if t.dim() >= 1 and t.numel() > CHUNK_ELEMS else None
    return [t] if rows is None else list(t.split(rows, 0))


def load_chunks(arrays, key):
    """The inverse of row_chunks over a {name: array} archive."""
    import numpy as np
    if key in arrays:
        return arrays[key]
    parts = []
    while f"{key}#{len(parts)}" in arrays:
        parts.append(arrays[f"{key}#{len(parts)}"])
    if not parts:
        raise KeyError(key)
    return np.concatenate(parts, 0)


def grad_param_names(G):
    """The first (sorted) cross-attention to_kv / to_q weight and null_kv of the generator."""
    names = sorted(n for n, _ in G.named_parameters() if ".cross_attns." in n)
    return [next(n for n in names if n.endswith(s)) for s in ("attn.to_kv.weight", "attn.to_q.weight", "attn.null_kv")]


def run_generator(G, img, strings):
    """One validation forward and the backward of sum(gen_img * R): returns gen_img, global_text_tokens and the
    gradients of grad_param_names(G) and of the latent z the synthesis network receives."""
    seen = {}

    def grab(module, args):
        seen["z"] = args[0]
        args[0].retain_grad()

    G.zero_grad(set_to_none=True)
    G.requires_grad_(False)
    for m in (G.synthesis, G.mapping, G.ldm_adapter):
        m.requires_grad_(True)
    handle = G.synthesis.register_forward_pre_hook(grab)
    try:
        torch.manual_seed(123)                   # epsilon of the posterior sample
        out = G(img, list(strings), validation=True)
    finally:
        handle.remove()
    (out.gen_img * loss_weights(out.gen_img.shape).to(out.gen_img.device)).sum().backward()
    params = dict(G.named_parameters())
    res = {"gen_img": out.gen_img.detach(), "global_text_tokens": out.global_text_tokens.detach(),
           "grad/z": seen["z"].grad.detach()}
    for n in grad_param_names(G):
        res["grad/" + n] = params[n].grad.detach()
    return res
