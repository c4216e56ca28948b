"""Qwen2.5-VL vision tower golden vectors, generated FROM THE REFERENCE ITSELF.

Runs only in the build container (CPU): imports the reference tree with the small third-party stand-ins of
tests/golden/ref_stubs (torchvision's `normalize` only), saves a tiny random `Qwen2_5_VLForConditionalGeneration`
(tests/qwen_case.py: vision depth 4, hidden 320, 4 heads of 80, intermediate 172, out 128, full attention at blocks
1 and 3; a one-layer text model) to a local directory, builds the reference's
`networks.utils.vfms.qwen_utils.QwenVisionEncoder` on it, overwrites every vision weight with tests/det_init.py
(values depend only on the state-dict name and shape, so the tests rebuild the same tower from a config.json alone)
and runs `encode_image` with patch_from_layers [0, 2, -1], B = 2, scale_factor 1.0 on
  * 140^2 (grid 10: windows 64, 16, 16, 4; full-attention segments of 100),
  * 168^2 (grid 12: windows 64, 32, 32, 16),
  * 252^2 (grid 18: full-attention segments of 324 tokens, crossing query and key tiles), and
  * 280^2 with the equivariance prior's bicubic antialiased downscale (eq_scale_factor 0.5 -> 140^2).

transformers 5.x returns a BaseModelOutputWithPooling from the vision model where the reference (written for
4.50) expects the merged tensor; the maker wraps `vision_model` so the wrapper receives `pooler_output`. The
transformers version is recorded in the metadata: parity is pinned to that version's modeling code.

The reference's hooks return index 0 in merge-group order and block outputs in window order, as [B N, D]; the maker
un-permutes both to [B, gh gw, D] raster order with its own index arithmetic (merge-group order by construction,
window order from HF's `get_vision_window_index`). Stored per case: the merged (-1) tokens and the pooled output in
full; for index 0 and block 2 every 5th raster token (all channels) and the per-token L2 norms of all tokens; and
`e_bf16`, the relative L2 error of the same model under torch.autocast("cpu", bfloat16) against its own fp32 output
(per output), which bounds what a second, independent bf16 evaluation may differ by.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_qwen.py
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
from transformers import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration  # noqa: E402
from transformers.vision_utils import get_vision_window_index  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))           # tests/ (det_init, qwen_case)
sys.path.insert(0, os.path.join(HERE, "ref_stubs"))
sys.path.insert(0, REF)

from det_init import det_init  # noqa: E402
import qwen_case as qc  # noqa: E402

OUT = os.path.join(HERE, "qwen_golden.npz")
ROW_STRIDE = 5
torch.set_num_threads(int(os.environ.get("THREADS", "8")))
arrays, meta = {}, {"cases": [], "transformers": transformers.__version__, "row_stride": ROW_STRIDE}


def put(k, v):
    arrays[k] = v.detach().cpu().float().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


class MergedOutput(torch.nn.Module):
    """The vision model as the reference wrapper expects it: forward returns the merged tokens."""

    def __init__(self, visual):
        super().__init__()
        self.visual = visual
        self.blocks = visual.blocks
        self.patch_embed = visual.patch_embed

    def forward(self, *args, **kwargs):
        out = self.visual(*args, **kwargs)
        return out if isinstance(out, torch.Tensor) else out.pooler_output


def raster_ids(B, grid, order):
    """Raster token id (b g + py) g + px at every slot of the reference's 2-D hook outputs. order 'group': the
    reference's patchify order (merge units raster, 2 x 2 tokens inside); 'window': HF's window_index applied
    to the units."""
    uw = grid // 2
    units = torch.arange(uw * uw)
    if order == "window":
        thw = torch.tensor([[1, grid, grid]])
        units, _ = get_vision_window_index(thw, spatial_merge_size=2, window_size=qc.VISION_CFG["window_size"],
                                           patch_size=14)
    s = torch.arange(4)
    py = (units[:, None] // uw) * 2 + s[None] // 2
    px = (units[:, None] % uw) * 2 + s[None] % 2
    tok = (py * grid + px).reshape(-1)
    return (torch.arange(B)[:, None] * grid * grid + tok[None]).reshape(-1)


def to_raster(x2d, B, grid, order):
    out = torch.empty_like(x2d)
    out[raster_ids(B, grid, order)] = x2d
    return out.reshape(B, grid * grid, -1)


work = tempfile.mkdtemp(prefix="vfm_golden_qwen_")
vfm_dir = os.path.join(work, qc.VFM_DIRNAME)
torch.manual_seed(0)
config = Qwen2_5_VLConfig(vision_config=dict(qc.VISION_CFG), text_config=dict(qc.TEXT_CFG))
Qwen2_5_VLForConditionalGeneration(config).float().save_pretrained(vfm_dir)

from networks.utils.vfms.qwen_utils import QwenVisionEncoder  # noqa: E402

enc = QwenVisionEncoder(model_name=vfm_dir, conditional=False, label_type="cls2id", scale_factor=1.0,
                        patch_from_layers=list(qc.LAYERS), amp_enabled=False)
visual = enc.vision_model.float()
touched = det_init(visual)
meta["det_init_tensors"] = len(touched)
enc.vision_model = MergedOutput(visual)
enc.eval()


def run(img, eqs, prior):
    feats, pooled = enc.encode_image(img, eqs, prior)
    B = img.shape[0]
    grid = int(round((feats[0].shape[0] // B) ** 0.5))
    return [to_raster(feats[0], B, grid, "group"), to_raster(feats[1], B, grid, "window"), feats[2]], pooled.float()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


with torch.no_grad():
    for case in qc.CASES:
        name, res, eqs, prior = case["name"], case["res"], case["eq_scale"], case["prior"]
        img = qc.image(res, case["seed"])
        meta[f"{name}/img_sum"] = float(img.double().sum())
        feats, pooled = run(img, eqs, prior)
        grid = int(round(feats[0].shape[1] ** 0.5))
        _, cu = get_vision_window_index(torch.tensor([[1, grid, grid]]), spatial_merge_size=2,
                                        window_size=qc.VISION_CFG["window_size"], patch_size=14)
        assert (cu[1:] - cu[:-1]).tolist() == case["windows"], (name, (cu[1:] - cu[:-1]).tolist())
        # the reference's own autocast path runs on "cuda" only; the CPU equivalent measures the bf16 error
        with torch.autocast("cpu", dtype=torch.bfloat16):
            feats16, pooled16 = run(img, eqs, prior)
        for hname, f, f16 in zip(qc.HIDDEN_NAMES, feats, feats16):
            meta[f"{name}/{hname}/shape"] = list(f.shape)
            meta[f"{name}/{hname}/e_bf16"] = rel_l2(f16.float(), f)
            if hname == "merged":
                put(f"{name}/{hname}/rows", f)
            else:
                put(f"{name}/{hname}/rows", f[:, ::ROW_STRIDE])
                put(f"{name}/{hname}/norms", f.double().norm(dim=-1))
        meta[f"{name}/e_bf16"] = meta[f"{name}/merged/e_bf16"]
        put(f"{name}/pooled", pooled)
        meta["cases"].append(name)
        print(name, [tuple(f.shape) for f in feats], {h: f"{meta[f'{name}/{h}/e_bf16']:.2e}" for h in qc.HIDDEN_NAMES},
              flush=True)
import golden_io  # noqa: E402  (tests/golden_io.py: archives over 1 MiB are written as <stem>.partNN.npz)
PARTS = golden_io.save_parts(OUT, dict(arrays, meta=np.array(json.dumps(meta))))
print("wrote", OUT, sum(os.path.getsize(p) for p in PARTS), "bytes")
