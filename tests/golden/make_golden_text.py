"""SigLIP2 text conditioning golden vectors, generated FROM THE REFERENCE ITSELF.

Runs only in the build container (CPU, fp32): imports the reference tree with the third-party stand-ins of
tests/golden/ref_stubs, saves a tiny random HF `SiglipModel` (tests/text_case.py: text tower hidden 128, 2 heads
of 64, 2 layers, vocabulary 300; tests/net_cases.py's vision tower) to a local directory and builds on it

  * the reference's `networks.utils.vfms.siglip2_utils.SigLIP2Encoder(conditional=True, label_type='cls2text')`,
    every weight overwritten with tests/det_init.py, and runs `encode_text` on text_case.STRINGS: the ids, the
    masks, `seq_tokens` (all 64 rows) and `pooled` in fp32, and per output `e_bf16`, the relative L2 error of the
    same model under torch.autocast("cpu", bfloat16) against its own fp32 output;
  * the reference's `Generator` at the tests/net_cases.py scale with conditional=True, label_type='cls2text',
    use_cross_attn=True, weights from det_init (CrossAttention.to_out and the feed-forward's second projection
    are zero-initialised by default: the cross-attention branch would be a no-op): gen_img, global_text_tokens and
    the gradients of sum(gen_img * R) w.r.t. one cross-attention to_kv / to_q weight, one null_kv and the latent z
    the synthesis network receives (text_case.run_generator), all stored whole (the large ones in row blocks,
    text_case.row_chunks; golden_io splits the archive into parts). Per stored tensor also `e_bf16_max`: the same
    generator evaluated once more with its whole forward under torch.autocast("cpu", bfloat16) against its own
    fp32 result, as max |difference| / max |fp32| (the metric of the network parity tests) -- what a second,
    independent bf16 evaluation of these quantities may differ by.

The directory has no tokenizer files; the reference's `AutoTokenizer.from_pretrained` call is answered with
text_case.ByteTokenizer (the stand-in the package uses for a model directory without weights), so both sides
see the same ids. The transformers version is recorded in the metadata: parity is pinned to that version's
modeling code.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_text.py
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("VFM_REFERENCE", "/root/reference")
import transformers  # noqa: E402,F401  (import before the stubs: keeps its torchvision probe negative)
from transformers import SiglipConfig, SiglipModel  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))           # tests/ (det_init, net_cases, text_case)
sys.path.insert(0, os.path.join(HERE, "ref_stubs"))
sys.path.insert(0, REF)

from det_init import det_init  # noqa: E402
import text_case as tc  # noqa: E402

OUT = os.path.join(HERE, "text_golden.npz")
torch.set_num_threads(int(os.environ.get("THREADS", "8")))
arrays, meta = {}, {"transformers": transformers.__version__, "strings": list(tc.STRINGS)}


def put(k, v):
    arrays[k] = v.detach().cpu().float().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


work = tempfile.mkdtemp(prefix="vfm_golden_text_")
vfm_dir = os.path.join(work, tc.VFM_DIRNAME)
torch.manual_seed(0)
SiglipModel(SiglipConfig(text_config=dict(tc.TEXT_CFG), vision_config=dict(tc.VISION_CFG))).float().save_pretrained(vfm_dir)

import networks.utils.vfms.siglip2_utils as ref_siglip  # noqa: E402


class _Tokenizers:
    @staticmethod
    def from_pretrained(*args, **kwargs):
        return tc.ByteTokenizer()


ref_siglip.AutoTokenizer = _Tokenizers

# ------------------------------------------------------------ the encoder's text branch
enc = ref_siglip.SigLIP2Encoder(model_name=vfm_dir, conditional=True, label_type="cls2text", scale_factor=1.0,
                                patch_from_layers=[0, 1, -1], amp_enabled=False)
inner = getattr(enc.text_model, "text_model", enc.text_model)       # transformers 4 nests the transformer
touched = det_init(inner.float(), prefix="text_model.")
meta["det_init_text_tensors"] = len(touched)
meta["text_state_keys"] = sorted(inner.state_dict().keys())
enc.eval()
tok = enc.tokenizer(list(tc.STRINGS), padding="max_length", max_length=64, truncation=True, return_tensors="pt",
                    return_attention_mask=True)
arrays["ids"] = tok["input_ids"].numpy()
arrays["mask"] = tok["attention_mask"].numpy().astype(np.uint8)
with torch.no_grad():
    seq, pooled, mask = enc.encode_text(list(tc.STRINGS))
    assert torch.equal(mask, tok["attention_mask"].bool())
    with torch.autocast("cpu", dtype=torch.bfloat16):
        seq16, pooled16, _ = enc.encode_text(list(tc.STRINGS))
put("seq_tokens", seq)
put("pooled", pooled)
meta["seq_tokens/e_bf16"] = rel_l2(seq16.float(), seq)
meta["pooled/e_bf16"] = rel_l2(pooled16.float(), pooled)
print("encode_text", tuple(seq.shape), tuple(pooled.shape), mask.sum(1).tolist(),
      {k: f"{meta[k + '/e_bf16']:.2e}" for k in tc.TOKENS}, flush=True)

# ------------------------------------------------------------ the text-conditional generator
from networks.generator import Generator  # noqa: E402
from networks.utils.vfm_utils import VFMEncoder  # noqa: E402

# the reference Generator reads `self.vfm_encoder.text_model.config.hidden_size`, but its VFMEncoder keeps the
# tower one level down (`.encoder.text_model`); the attribute is supplied here so that the conditional generator
# can be built at all (the package reads `.encoder.text_model`)
VFMEncoder.text_model = property(lambda self: self.encoder.text_model)

G = Generator(label_dim=0, **tc.g_kwargs(vfm_dir)).train()
det_init(G)
meta["G_state_keys"] = sorted(G.state_dict().keys())
meta["G_grad_names"] = tc.grad_param_names(G)
res = tc.run_generator(G, tc.image(), tc.STRINGS)
G.mapping.eval()      # its train-mode x_avg update lerps a bf16 mean into the fp32 buffer (a dtype error under
#                       autocast); the update is a side effect on a buffer, not part of any output
with torch.autocast("cpu", dtype=torch.bfloat16):
    res16 = {k: v.float() for k, v in tc.run_generator(G, tc.image(), tc.STRINGS).items()}
for k, v in res.items():
    meta[f"G/{k}/norm"] = float(v.double().norm())
    m = float(v.abs().max())
    meta[f"G/{k}/e_bf16_max"] = float((res16[k].double() - v.double()).abs().max() / m) if m > 0 else 0.0
    chunks = tc.row_chunks(v)
    for i, c in enumerate(chunks):
        put(f"G/{k}" if len(chunks) == 1 else f"G/{k}#{i}", c)
    print("G/" + k, tuple(v.shape), f"max |.| {m:.3e}", f"e_bf16_max {meta[f'G/{k}/e_bf16_max']:.2e}", flush=True)

import golden_io  # noqa: E402  (tests/golden_io.py: archives over 1 MiB are written as <stem>.partNN.npz)
PARTS = golden_io.save_parts(OUT, dict(arrays, meta=np.array(json.dumps(meta))))
print("wrote", OUT, sum(os.path.getsize(p) for p in PARTS), "bytes")
