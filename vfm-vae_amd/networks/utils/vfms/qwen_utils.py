"""Frozen Qwen2.5-VL vision tower as a VFM backbone.

Replaces the reference wrapper `networks/utils/vfms/qwen_utils.py:29-261`, which loads
`transformers.Qwen2_5_VLForConditionalGeneration.from_pretrained(name)`, keeps its `visual` tower and runs
it under bf16 autocast. The module tree and state-dict keys are HF's
(`patch_embed.proj`, `blocks.N.{norm1, norm2, attn.{qkv, proj}, mlp.{gate_proj, up_proj, down_proj}}`,
`merger.{ln_q, mlp.0, mlp.2}`), so a local HF directory (config.json + *.safetensors, keys prefixed
`visual.` or `model.visual.`; the language model's tensors are dropped) loads unchanged. Without one the
7B tower's architecture is random-initialised from a fixed seed (no network here).

Math = HF `Qwen2_5_VisionTransformerPretrainedModel.forward` under autocast(bf16):
  preprocess  uint8 -> [0, 1], optional bicubic antialiased eq-downscale, bicubic resize by scale_factor,
              CLIP mean / std (reference :114-137);
  patchify    each 14 x 14 patch is one row; the reference duplicates the single frame over the temporal
              pair (:162-169), so the Conv3d's two temporal weight slices see the same pixels and are folded
              into one [D, 588] matrix (K padded to 640 with zero columns for the GEMM tiles);
  order       the reference groups patches by 2 x 2 merge unit (:177-192) and HF permutes the units into
              window order (`get_vision_window_index`: 4 x 4 units = 64 tokens per window, smaller at the
              edges, empty ones dropped). One gather takes the image straight to window order
              (`window_layout`); the intermediate orders are never materialised;
  block       h += proj(attn(rmsnorm1(h))); n = rmsnorm2(h); h += down(silu(gate(n)) * up(n)); eps 1e-6;
              blocks in `fullatt_block_indexes` attend over the whole image, the others inside their window
              (a `cu_seqlens` list per regime, built once per geometry and kept on the device);
  rope        table of head_dim/2 entries (row-position frequencies, then column-position ones) duplicated
              to head_dim; x cos + rotate_half(x) sin in fp32, rounded to the compute dtype before QK^T;
  dtypes      the residual stream is in the compute dtype (bf16 under autocast: unlike the fp32 streams of
              the other towers here), RMSNorm computes in fp32 and emits the compute dtype, softmax is fp32,
              silu(gate) is rounded before the product with up;
  merger      rmsnorm, the four tokens of a merge unit concatenated, Linear -> erf-GELU -> Linear, then the
              inverse window permutation: [B, (gh/2)(gw/2), out_hidden] in raster order.
Compute dtype = amp_dtype if (amp_enabled and the input is on a ROCm device) else fp32, as in the other
towers. On ROCm under bf16 every op is one of this project's kernels (vit_ops: gemm9 products with bias /
erf-GELU epilogues on zero-padded cached weights, csrc/qwen.hip for the rest).

Two places where the reference cannot be followed literally:

  * Intermediate layers. The reference's forward hooks return index 0 and block outputs as 2-D [B N, D]
    tensors, index 0 in merge-group order and block outputs in window order, and the fusion adapter then
    reshapes by int(N ** 0.5): it cannot consume them. Here they come back as [B, gh gw, D] in row-major
    raster order of the patch grid; the values are the reference's.
  * Token grid. The reference Generator computes `patch_resolutions` from patch_size = 14
    (generator.py:1007), but index -1 yields the merged grid, half of that, so the adapter's down-scale
    factors are wrong for it. `patch_size` stays 14; the encoder additionally carries `token_strides`, a
    list aligned with `patch_from_layers` (28 for -1, else 14), which the Generator uses when present.
"""
import re
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from torch_utils import distributed as dist
from torch_utils.ops import vit_ops
from .vit_tower import Linear, load_safetensors_dir, local_config, seeded_init

_QWEN_7B = dict(depth=32, hidden_size=1280, num_heads=16, intermediate_size=3420, out_hidden_size=3584,
                window_size=112, fullatt_block_indexes=[7, 15, 23, 31], patch_size=14, spatial_merge_size=2,
                temporal_patch_size=2, in_channels=3)


def qwen_config_from_name(model_name):
    """Vision dimensions from a local HF directory's `vision_config`, else the 7B tower's."""
    cfg = dict(_QWEN_7B)
    local = local_config(model_name)
    if local is not None:
        cfg.update({k: local[k] for k in _QWEN_7B if k in local})
    if cfg["hidden_size"] % cfg["num_heads"] or (cfg["hidden_size"] // cfg["num_heads"]) % 4:
        raise ValueError(f"Qwen vision tower: hidden {cfg['hidden_size']} / heads {cfg['num_heads']} is not a "
                         "rotary head dim (a multiple of 4)")
    if cfg["temporal_patch_size"] != 2 or cfg["in_channels"] != 3:
        raise NotImplementedError("Qwen vision tower: only single RGB frames (temporal_patch_size 2) are supported")
    return cfg


def _pad64(n):
    return (n + 63) // 64 * 64


def window_layout(B, gh, gw, merge=2, window_units=4):
    """Index arithmetic of the tower's token order for B images of gh x gw patches.

    Returns (win2raster, unit_win2raster, window_lengths, rows, cols):
      win2raster       long [B gh gw]: raster patch id (b gh + py) gw + px of the token at each window-order slot;
      unit_win2raster  long [B gh gw / 4]: the same for merge units ((b uh + uy) uw + ux), = HF's window_index;
      window_lengths   token count of every non-empty window, in order (all images);
      rows, cols       long [B gh gw]: py, px of each window-order token (the rotary positions).
    Window order: windows row-major over the unit grid, units row-major inside a window, the merge * merge
    tokens of a unit row-major inside it."""
    uh, uw = gh // merge, gw // merge
    uy, ux = torch.meshgrid(torch.arange(uh), torch.arange(uw), indexing="ij")
    nww = -(-uw // window_units)
    wid = ((uy // window_units) * nww + ux // window_units).reshape(-1)
    order = torch.argsort(wid, stable=True)                    # raster unit id at each window-order unit slot
    lengths = (torch.bincount(wid) * merge * merge).tolist()
    lengths = [n for n in lengths if n > 0]
    uyo, uxo = order // uw, order % uw
    s = torch.arange(merge * merge)
    py = (uyo[:, None] * merge + s[None] // merge).reshape(-1)
    px = (uxo[:, None] * merge + s[None] % merge).reshape(-1)
    tok = py * gw + px
    b = torch.arange(B)[:, None]
    win2raster = (b * (gh * gw) + tok[None]).reshape(-1)
    unit_win2raster = (b * (uh * uw) + order[None]).reshape(-1)
    return win2raster, unit_win2raster, lengths * B, py.repeat(B), px.repeat(B)


class _Geometry:
    """Device-resident index tables of one (B, gh, gw): built once, reused by every forward."""

    def __init__(self, B, gh, gw, head_dim, device, merge=2, window_units=4, theta=10000.0):
        w2r, u_w2r, lengths, py, px = window_layout(B, gh, gw, merge, window_units)
        self.gather = w2r.to(torch.int32).to(device)                 # patch gather: image -> window order
        self.to_raster = torch.argsort(w2r).to(device)               # window-order rows -> raster rows
        self.units_to_raster = torch.argsort(u_w2r).to(device)       # HF reverse_indices
        self.window = vit_ops.Segments(lengths, device)
        self.full = vit_ops.Segments([gh * gw] * B, device)
        # HF Qwen2_5_VisionRotaryEmbedding(head_dim // 2): inv_freq over head_dim / 4 entries, (row, col) x freq
        dim = head_dim // 2
        inv_freq = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float) / dim))
        pos = torch.stack([py, px], -1)                              # [T, 2]
        emb = (pos.unsqueeze(-1) * inv_freq).flatten(1)              # [T, head_dim / 2]
        emb = torch.cat((emb, emb), -1)
        self.cos = emb.cos().contiguous().to(device)
        self.sin = emb.sin().contiguous().to(device)


class RMSNorm(nn.Module):
    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps


class _PatchEmbed(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        p, t = cfg["patch_size"], cfg["temporal_patch_size"]
        self.proj = nn.Conv3d(cfg["in_channels"], cfg["hidden_size"], kernel_size=(t, p, p), stride=(t, p, p),
                              bias=False)


class _Attention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        d = cfg["hidden_size"]
        self.heads = cfg["num_heads"]
        self.qkv = Linear(d, 3 * d)
        self.proj = Linear(d, d)

    def forward(self, y, geo, seg):
        return self.proj(vit_ops.rope_attention_varlen(self.qkv(y), geo.cos, geo.sin, seg, self.heads))


def _cached(owner, name, params, dtype, build):
    """`build()` cached on `owner` until a source parameter's storage or version moves (frozen tower: once)."""
    key = (dtype,) + tuple((p.data_ptr(), p._version) for p in params)
    capturing = params[0].is_cuda and torch.cuda.is_current_stream_capturing()
    hit = owner.__dict__.get(name)
    if hit is not None and hit[0] == key and not capturing:
        return hit[1]
    val = build()
    if not torch.is_grad_enabled() and not capturing:
        owner.__dict__[name] = (key, val)
    return val


class _MLP(nn.Module):
    """SwiGLU MLP. The GEMMs run on zero-padded copies of the frozen weights (intermediate width I -> Ip, the
    next multiple of 64, which the 256-tile GEMM's K tiling needs): gate | up as one [2 Ip, D] product, down as
    [D, Ip]. The pad rows / columns and pad biases are zero, so the padded activations are exactly zero and add
    exactly nothing to the down projection."""

    def __init__(self, cfg):
        super().__init__()
        d, i = cfg["hidden_size"], cfg["intermediate_size"]
        self.inter = i
        self.gate_proj = nn.Linear(d, i)
        self.up_proj = nn.Linear(d, i)
        self.down_proj = nn.Linear(i, d)

    def _padded(self, dtype):
        g, u, dn = self.gate_proj, self.up_proj, self.down_proj

        def build():
            i, ip, d = self.inter, _pad64(self.inter), g.weight.shape[1]
            w = g.weight.new_zeros(2 * ip, d)
            w[:i], w[ip:ip + i] = g.weight, u.weight
            b = g.bias.new_zeros(2 * ip)
            b[:i], b[ip:ip + i] = g.bias, u.bias
            wd = dn.weight.new_zeros(d, ip)
            wd[:, :i] = dn.weight
            return w.to(dtype), b, wd.to(dtype)
        return _cached(self, "_vfm_padded", (g.weight, u.weight, dn.weight, g.bias, u.bias), dtype, build)

    def forward(self, n):
        w, b, wd = self._padded(n.dtype)
        a = vit_ops.swiglu(vit_ops.linear(n, w, b), self.inter)
        return vit_ops.linear(a, wd, self.down_proj.bias)


class QwenVisionBlock(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.norm1 = RMSNorm(cfg["hidden_size"])
        self.norm2 = RMSNorm(cfg["hidden_size"])
        self.attn = _Attention(cfg)
        self.mlp = _MLP(cfg)

    def forward(self, h, y, geo, seg, next_norm):
        """h: the stream, y = norm1(h). Returns (h after the block, next_norm(h) or None): each residual add is
        fused with the norm that reads its result."""
        h, n = vit_ops.residual_rms_norm(h, self.attn(y, geo, seg), self.norm2.weight, self.norm2.eps)
        return vit_ops.residual_rms_norm(h, self.mlp(n), None if next_norm is None else next_norm.weight,
                                         1e-6 if next_norm is None else next_norm.eps)


class _Merger(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        d = cfg["hidden_size"] * cfg["spatial_merge_size"] ** 2
        self.ln_q = RMSNorm(cfg["hidden_size"])
        self.mlp = nn.Sequential(Linear(d, d), nn.GELU(), Linear(d, cfg["out_hidden_size"]))

    def forward(self, y):
        """y = ln_q(h) [T, D] in window order -> [T / 4, out] (window-unit order)."""
        fc1, fc2 = self.mlp[0], self.mlp[2]
        y = y.reshape(-1, fc1.in_features)
        return fc2(vit_ops.linear_gelu(y, vit_ops.frozen_weight(fc1.weight, y.dtype), fc1.bias))


class QwenVisionTower(nn.Module):
    """HF Qwen2_5_VisionTransformerPretrainedModel-compatible container (single frames)."""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.patch_embed = _PatchEmbed(cfg)
        self.blocks = nn.ModuleList([QwenVisionBlock(cfg) for _ in range(cfg["depth"])])
        self.merger = _Merger(cfg)
        self.head_dim = cfg["hidden_size"] // cfg["num_heads"]
        self.window_units = cfg["window_size"] // cfg["spatial_merge_size"] // cfg["patch_size"]
        self._geo = {}

    def reset_parameters(self, seed=1234):
        g = seeded_init(self, seed)
        with torch.no_grad():
            w = self.patch_embed.proj.weight
            w.copy_(torch.randn(w.shape, generator=g) / (w[0].numel() ** 0.5))

    def geometry(self, B, gh, gw, device):
        key = (B, gh, gw, str(device))
        geo = self._geo.get(key)
        if geo is None:
            if len(self._geo) >= 8:
                self._geo.clear()
            geo = self._geo[key] = _Geometry(B, gh, gw, self.head_dim, device, self.config["spatial_merge_size"],
                                             self.window_units)
        return geo

    def patch_weight(self, dtype):
        """[D, Kp] patch projection: the two temporal slices summed (both see the same frame), K = 588 -> 640."""
        w = self.patch_embed.proj.weight

        def build():
            w2 = w.sum(2).reshape(w.shape[0], -1)
            return F.pad(w2, (0, _pad64(w2.shape[1]) - w2.shape[1])).to(dtype).contiguous()
        return _cached(self.patch_embed, "_vfm_folded", (w,), dtype, build)

    @torch.no_grad()
    def forward_features(self, pixel_values, want: List[int], want_last: bool, compute_dtype):
        """pixel_values: normalised fp32 [B, 3, H, W]. Returns ({i: [B, gh gw, D] raster order} for i in want:
        0 = patch embedding, i = output of block i; merged [B, gh gw / 4, out] raster order or None)."""
        cfg = self.config
        B, _, H, W = pixel_values.shape
        p, m = cfg["patch_size"], cfg["spatial_merge_size"]
        gh, gw = H // p, W // p
        if H % p or W % p or gh % m or gw % m:
            raise ValueError(f"Qwen vision tower: {H} x {W} is not a whole number of {m} x {m} groups of {p}-pixel patches")
        geo = self.geometry(B, gh, gw, pixel_values.device)
        wp = self.patch_weight(compute_dtype)
        rows = vit_ops.patch_rows(pixel_values.float(), geo.gather, p, wp.shape[1], compute_dtype)
        h = vit_ops.linear(rows, wp)                                           # [T, D], window order
        raster = lambda t: t.index_select(0, geo.to_raster).reshape(B, gh * gw, -1)
        saved = {0: raster(h)} if 0 in want else {}
        n = len(self.blocks)
        last_needed = n if want_last else max([i for i in want if i > 0], default=0)
        if last_needed:
            y = vit_ops.rms_norm(h, self.blocks[0].norm1.weight, self.blocks[0].norm1.eps)
        for i, blk in enumerate(self.blocks[:last_needed], start=1):
            nxt = self.blocks[i].norm1 if i < last_needed else (self.merger.ln_q if want_last else None)
            seg = geo.full if (i - 1) in cfg["fullatt_block_indexes"] else geo.window
            h, y = blk(h, y, geo, seg, nxt)
            if i in want:
                saved[i] = raster(h)
        merged = None
        if want_last:
            if not last_needed:
                y = vit_ops.rms_norm(h, self.merger.ln_q.weight, self.merger.ln_q.eps)
            merged = self.merger(y).index_select(0, geo.units_to_raster).reshape(B, gh * gw // (m * m), -1)
        return saved, merged


class QwenVisionEncoder(nn.Module):
    """Reference interface: encode_image(img, eq_scale_factor, is_eq_prior) -> (patch_features, pooled)."""

    def __init__(self, model_name: str, conditional: bool = False, label_type: str = "cls2id",
                 scale_factor: float = 1.0, patch_from_layers: List[int] = (-1,),
                 amp_dtype: torch.dtype = torch.bfloat16, amp_enabled: bool = True):
        super().__init__()
        self.model_name = model_name
        self.conditional = conditional
        self.label_type = label_type
        self.scale_factor = scale_factor
        self.patch_from_layers = list(patch_from_layers)
        self.amp_dtype = amp_dtype
        self.amp_enabled = amp_enabled
        if conditional and label_type in ["text", "cls2text"]:
            raise NotImplementedError("Qwen2.5-VL text conditioning needs the HF language model and tokenizer, "
                                      "which are not part of the MI355X training path")
        cfg = qwen_config_from_name(model_name)
        self.patch_size = cfg["patch_size"]
        self.merge_size = cfg["spatial_merge_size"]
        self.temporal_patch_size = cfg["temporal_patch_size"]
        # pixels per token along each axis, aligned with patch_from_layers: -1 is the merged grid
        self.token_strides = [self.patch_size * (self.merge_size if i == -1 else 1) for i in self.patch_from_layers]
        n = cfg["depth"]
        for i in self.patch_from_layers:
            if not (-n - 1 <= i <= n):
                raise ValueError(f"Layer index {i} is out of range for {n} blocks.")
        self.register_buffer("_mean", torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 3, 1, 1),
                             persistent=False)
        self.register_buffer("_std", torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 3, 1, 1),
                             persistent=False)
        self.vision_model = QwenVisionTower(cfg)
        self.vision_model.reset_parameters()

        def rename(k):
            m = re.match(r"^(?:model\.)?visual\.(.*)$", k)
            return m.group(1) if m else None                  # language model / lm_head tensors are dropped
        loaded = load_safetensors_dir(self.vision_model, model_name, rename=rename)
        self.vision_model.eval().requires_grad_(False)
        self.pretrained_loaded = loaded
        self.tokenizer = None
        self.text_model = None
        self.use_text = False
        dist.print0(f"QwenVisionEncoder ready: {model_name} ({'pretrained' if loaded else 'random init'}), "
                    f"{cfg['depth']} blocks, hidden {cfg['hidden_size']}, heads {cfg['num_heads']}, "
                    f"out {cfg['out_hidden_size']}, full attention at {cfg['fullatt_block_indexes']}, "
                    f"layers {self.patch_from_layers}, scale_factor {scale_factor}")

    def _preprocess_image(self, img, eq_scale_factor, is_eq_prior):
        if img.dtype == torch.uint8:
            img = img.float() / 255.0
        if is_eq_prior and eq_scale_factor < 1.0:
            img = F.interpolate(img, scale_factor=eq_scale_factor, mode="bicubic", align_corners=False, antialias=True)
        if self.scale_factor != 1.0:
            img = F.interpolate(img, scale_factor=self.scale_factor, mode="bicubic", align_corners=False,
                                antialias=(self.scale_factor < 1.0))
        return (img - self._mean.to(img.device)) / self._std.to(img.device)

    @torch.no_grad()
    def encode_image(self, img, eq_scale_factor=1.0, is_eq_prior=False):
        x = self._preprocess_image(img, eq_scale_factor, is_eq_prior)
        dtype = self.amp_dtype if (self.amp_enabled and x.is_cuda) else torch.float32
        n = len(self.vision_model.blocks)
        idx = [i if i >= 0 else n + i + 2 for i in self.patch_from_layers if i != -1]
        saved, merged = self.vision_model.forward_features(x, idx, want_last=True, compute_dtype=dtype)
        feats = []
        for i in self.patch_from_layers:
            feats.append((merged if i == -1 else saved[i if i >= 0 else n + i + 2]).float())
        return feats, merged.float().mean(dim=1)

    @torch.no_grad()
    def encode_text(self, text):
        return None, None, None
