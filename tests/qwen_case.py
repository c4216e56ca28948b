"""The tiny Qwen2.5-VL vision tower shared by tests/golden/make_golden_qwen.py (reference side) and the Qwen
tests (this package): depth 4, hidden 320, 4 heads (head dim 80), intermediate 172 (not a multiple of 64: the
zero-padded GEMM operands), out 128, full attention at blocks 1 and 3, windows of 4 x 4 merge units."""
import torch

VFM_DIRNAME = "tiny-qwen2.5-vl"
VISION_CFG = dict(depth=4, hidden_size=320, num_heads=4, intermediate_size=172, out_hidden_size=128,
                  fullatt_block_indexes=[1, 3], window_size=112, patch_size=14, spatial_merge_size=2,
                  temporal_patch_size=2, in_channels=3, hidden_act="silu")
# one-layer text model (only there so that Qwen2_5_VLForConditionalGeneration can be built and saved)
TEXT_CFG = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
                intermediate_size=64, vocab_size=64, max_position_embeddings=128)
LAYERS = (0, 2, -1)               # patch embedding, output of block 2 (index 1, a full-attention block), merger
HIDDEN_NAMES = ("h0", "h2", "merged")
BATCH = 2
# window token counts per image (checked against HF get_vision_window_index by the maker and the CPU test)
CASES = (dict(name="r140", res=140, eq_scale=1.0, prior=False, seed=41, windows=[64, 16, 16, 4]),
         dict(name="r168", res=168, eq_scale=1.0, prior=False, seed=42, windows=[64, 32, 32, 16]),
         dict(name="r252", res=252, eq_scale=1.0, prior=False, seed=43,
              windows=[64, 64, 16, 64, 64, 16, 16, 16, 4]),
         dict(name="r280eq", res=280, eq_scale=0.5, prior=True, seed=44, windows=[64, 16, 16, 4]))


def image(res, seed, batch=BATCH):
    """A [batch, 3, res, res] input in [0, 1] from a seeded CPU generator (the same values on every machine)."""
    return torch.rand(batch, 3, res, res, generator=torch.Generator().manual_seed(seed))
