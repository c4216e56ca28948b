"""VFM encoder dispatch (reference `networks/utils/vfm_utils.py:26-123`).

Index convention of `patch_from_layers` (shared by every backbone):
  0 = output of the patch embedding, i = output of block i,
 -1 = final sequence after the post-norm, -2 = last block, -3 = second-last, ...
"""
from typing import List

import torch
import torch.nn as nn

from .vfms.siglip2_utils import SigLIP2Encoder

VFM2INTERPOLATION = {
    'siglip': 'bilinear',
    'qwen': 'bicubic',
    'dino': 'bicubic',
    'mae': 'bilinear',
    'eva': 'bicubic',
    'clip': 'bicubic',
}


class VFMEncoder(nn.Module):
    def __init__(self, model_name: str, conditional: bool, label_type: str, scale_factor: float,
                 patch_from_layers: List[int], amp_dtype: torch.dtype = torch.bfloat16, amp_enabled: bool = True):
        super().__init__()
        name = model_name.lower()
        if "siglip2" in name:
            self.encoder = SigLIP2Encoder(model_name=model_name, conditional=conditional, label_type=label_type,
                                          scale_factor=scale_factor, patch_from_layers=patch_from_layers,
                                          amp_dtype=amp_dtype, amp_enabled=amp_enabled)
        elif "dinov2" in name:
            from .vfms.dinov2_utils import DINOv2Encoder
            self.encoder = DINOv2Encoder(model_name=model_name, patch_from_layers=patch_from_layers,
                                         scale_factor=scale_factor, amp_dtype=amp_dtype, amp_enabled=amp_enabled)
        elif "clip" in name:
            from .vfms.clip_utils import CLIPVisionEncoder
            self.encoder = CLIPVisionEncoder(model_name=model_name, patch_from_layers=patch_from_layers,
                                             scale_factor=scale_factor, amp_dtype=amp_dtype, amp_enabled=amp_enabled)
        elif "qwen" in name:
            from .vfms.qwen_utils import QwenVisionEncoder
            self.encoder = QwenVisionEncoder(model_name=model_name, conditional=conditional, label_type=label_type,
                                             scale_factor=scale_factor, patch_from_layers=patch_from_layers,
                                             amp_dtype=amp_dtype, amp_enabled=amp_enabled)
        else:
            raise NotImplementedError(
                f"VFM backbone '{model_name}' is not part of the MI355X training path "
                "(supported: siglip2, dinov2, clip, qwen)")

    @property
    def patch_size(self) -> int:
        return self.encoder.patch_size

    @property
    def token_strides(self):
        """Pixels per token of each `patch_from_layers` entry, for backbones whose outputs do not all live on
        the patch grid (Qwen2.5-VL: the merged -1 output); None: every entry is on the patch_size grid."""
        return getattr(self.encoder, "token_strides", None)

    # ------------------------------------------------------------------ feature reuse
    # The frozen tower runs once per phase on the same microbatch (reference loss.py: the D
    # phase's no-grad run_G and the G phase's run_G both encode real_img). Its output depends
    # only on the image and on the input transform the equivariance draw selects, so when the
    # G phase draws the same transform as the D phase the features are reused: exact, and one
    # full ViT forward less per iteration. Enabled by TotalLoss; one entry, consumed once.

    reuse_features = False
    last_features = None

    @staticmethod
    def input_transform(eq_scale_factor, is_eq_prior):
        """Canonical form of what the tower sees: only a prior draw with scale < 1 resizes."""
        return float(eq_scale_factor) if (is_eq_prior and eq_scale_factor < 1.0) else 1.0

    def offer_features(self, img, transform, feats, pooled):
        """Register features of `img` under `transform` (held with a reference to img, so the
        identity key cannot be recycled while the entry lives). One entry per microbatch image:
        with gradient accumulation every D-phase microbatch offers its own."""
        reg = self.__dict__.setdefault('_reuse', {})
        reg[id(img)] = (img, img._version, transform, feats, pooled)

    def clear_features(self):
        self.__dict__.setdefault('_reuse', {}).clear()
        self.last_features = None

    def _take(self, img, transform):
        """The features offered for exactly this image tensor (same object, same version) under the
        same input transform, consumed on a match; entries of other images are left alone."""
        reg = self.__dict__.get('_reuse')
        e = reg.get(id(img)) if reg else None
        if e is None:
            return None
        src, ver, tr, feats, pooled = e
        if src is not img or ver != img._version:
            del reg[id(img)]                     # stale (the tensor changed since it was offered)
            return None
        if tr != transform:
            return None
        del reg[id(img)]
        self.reuse_hits = getattr(self, 'reuse_hits', 0) + 1
        return feats, pooled

    def encode_image(self, img, eq_scale_factor: float = 1.0, is_eq_prior: bool = False):
        if not self.reuse_features:
            return self.encoder.encode_image(img, eq_scale_factor, is_eq_prior)
        transform = self.input_transform(eq_scale_factor, is_eq_prior)
        hit = self._take(img, transform)
        if hit is not None:
            return hit
        feats, pooled = self.encoder.encode_image(img, eq_scale_factor, is_eq_prior)
        self.last_features = (transform, feats, pooled)    # graph capture reads its static outputs here
        return feats, pooled

    def encode_text(self, text):
        return self.encoder.encode_text(text)
