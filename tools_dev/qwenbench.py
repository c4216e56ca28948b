"""Forward time of the frozen Qwen2.5-VL vision tower (networks/utils/vfms/qwen_utils.py) at the 7B dimensions
(32 blocks, hidden 1280, 16 heads of 80, intermediate 3420, out 3584), bf16, 448^2 input: this project's kernels
(gemm9 products on zero-padded weights, csrc/qwen.hip for attention / RMSNorm / SwiGLU / patch gather) against the
torch formulation of the same module (library GEMMs, per-segment SDPA batched over equal-length segments, torch
RMSNorm / SiLU), alternating the two in one process. Then the kernel timer's per-region totals of one forward on
the own path, with the attention kernel's rate over the windowed and full layers.

  python tools_dev/qwenbench.py [--batch 32] [--depth 32] [--iters 5] [--rounds 3]

Times are device-event intervals around whole forwards (encode_image on a resident fp32 image batch) that end in a
synchronise. Weights are random (fixed seed); the values do not change the work."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vfm-vae_amd"), ROOT]
import torch  # noqa: E402

from torch_utils.ops import kernel_timer, vit_ops  # noqa: E402
from networks.utils.vfms.qwen_utils import QwenVisionEncoder  # noqa: E402


def set_path(own):
    vit_ops.OWN_GEMM = own
    vit_ops.QWEN_OWN = own


def timed(fn, iters):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--res", type=int, default=448)
    ap.add_argument("--out", default=None, help="write the result JSON here as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("qwenbench needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    d = tempfile.mkdtemp(prefix="qwenbench_")
    full = [i for i in (7, 15, 23, 31) if i < a.depth] or [a.depth - 1]
    json.dump(dict(vision_config=dict(depth=a.depth, fullatt_block_indexes=full)),
              open(os.path.join(d, "config.json"), "w"))
    enc = QwenVisionEncoder(model_name=d, scale_factor=1.0, patch_from_layers=[-1]).eval().to(dev)
    img = torch.rand(a.batch, 3, a.res, a.res, generator=torch.Generator().manual_seed(0)).to(dev)
    run = lambda: enc.encode_image(img)
    outs = {}
    for own in (True, False):                    # warm both paths (weight casts, padded copies, library tuning)
        set_path(own)
        for _ in range(2):
            outs[own] = run()[0][0]
    diff = float((outs[True].double() - outs[False].double()).norm() / outs[False].double().norm())
    times = {True: [], False: []}
    for _ in range(a.rounds):
        for own in (True, False):
            set_path(own)
            times[own].append(timed(run, a.iters))
    set_path(True)
    kernel_timer.enable(True)
    run()
    summ = kernel_timer.summary()
    kernel_timer.enable(False)
    # attention workgroup size A/B (VFM_QWEN_ATTN_WAVES) on the kernel alone, per regime: one windowed and one
    # full-image call on a random packed projection of the tower's shape, device events over 20 calls
    from torch_utils.ops import qwen_hip
    g = a.res // 14
    geo = enc.vision_model.geometry(a.batch, g, g, dev)
    heads = enc.vision_model.config["num_heads"]
    qkv = torch.randn(a.batch * g * g, 3 * heads * 80, device=dev).to(torch.bfloat16)
    attn_ab = {"window": {}, "full": {}}
    for waves in ("1", "2", "4", "8"):
        os.environ["VFM_QWEN_ATTN_WAVES"] = waves
        for regime, seg in (("window", geo.window), ("full", geo.full)):
            call = lambda: qwen_hip.rope_attention_varlen(qkv, geo.cos, geo.sin, seg.cu, heads, seg.max_len)
            call()
            attn_ab[regime][waves] = [round(timed(call, 20) * 1e3, 1) for _ in range(3)]
    os.environ.pop("VFM_QWEN_ATTN_WAVES")
    regions = {k: dict(launches=v["launches"], total_ms=round(v["total_ms"], 3),
                       tflops=round(v["flops"] / v["total_ms"] / 1e9, 1) if v["flops"] else None,
                       gbs=round(v["bytes"] / v["total_ms"] / 1e6, 1) if v["bytes"] else None)
               for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["total_ms"])}
    res = dict(batch=a.batch, res=a.res, depth=a.depth, tokens=a.batch * (a.res // 14) ** 2,
               own_ms=[round(t, 2) for t in times[True]], torch_ms=[round(t, 2) for t in times[False]],
               own_ms_median=round(sorted(times[True])[len(times[True]) // 2], 2),
               torch_ms_median=round(sorted(times[False])[len(times[False]) // 2], 2),
               rel_l2_own_vs_torch=diff, kernel_ms_one_forward=round(sum(v["total_ms"] for v in summ.values()), 2),
               regions=regions, attention_us_per_call_by_forced_waves=attn_ab,
               note="rope_attention_varlen flops count max_seqlen keys per query (64 on windowed layers, the whole "
                    "image on full ones); its region sums both regimes")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
