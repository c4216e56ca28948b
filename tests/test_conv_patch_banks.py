"""Host check of the patch-staged conv's LDS image (csrc/conv.hip conv3x3_patch_kernel) through
tools_dev/conv_patch_banks.py: with the kernel's row pitch every A fragment is read from where the staging wrote
it, and every ds_read_b128 / ds_write_b64 lane group is bank-conflict-free for all nine tap shifts. No GPU."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("conv_patch_banks", os.path.join(ROOT, "tools_dev", "conv_patch_banks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_patch_image_is_consistent_and_conflict_free():
    src = open(os.path.join(ROOT, "vfm-vae_amd", "csrc", "conv.hip"), encoding="utf-8").read()
    pitch = int(re.search(r"constexpr int PPITCH = (\d+);", src).group(1))
    pt = int(re.search(r"constexpr int PT = (\d+);", src).group(1))
    tool = _tool()
    assert pt == tool.PT
    assert tool.check(pitch) == (1, 1)
    # the unpadded pitch (18 rows) is not: the padding is what makes the reads conflict-free
    assert tool.check(tool.PHALO)[0] > 1
