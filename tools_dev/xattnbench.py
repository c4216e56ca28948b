"""A/B of the text-conditioning kernels (csrc/xattn.hip) against the torch formulation on the same commit:

  * the decoder's CrossAttention module, forward + backward, at the three decoder shapes (B = 32, 8 heads of 64,
    64 text tokens of width 1024, 8 x 8 / 16 x 16 / 32 x 32 queries): VFM_XATTN=hip (projections, masked attention
    and output projection as one Function) against VFM_XATTN=torch (q.contiguous(), two torch.cat, the expanded
    boolean mask, F.scaled_dot_product_attention);
  * the SigLIP2-large text tower (24 layers, hidden 1024, 16 heads of 64) at B = 32 under bf16: own GEMMs + the
    key-masked attention kernel against hipBLASLt GEMMs + SDPA with the mask (VFM_VIT_GEMM=torch).

Each figure is the median of REPEATS timed runs of ITERS calls after WARM untimed ones, with the min - max spread of
the runs; the two routes alternate run by run, so drift hits both alike.
  python tools_dev/xattnbench.py [--out profiles/NAME.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vfm-vae_amd"), ROOT]
import torch  # noqa: E402

from networks.utils.gigagan_utils import CrossAttention  # noqa: E402
from networks.utils.vfms.siglip2_utils import ByteTokenizer, SiglipTextModel, siglip_text_config_from_name  # noqa: E402
from torch_utils.ops import vit_ops, xattn_hip  # noqa: E402

WARM, ITERS, REPEATS = 5, 10, 9
DEV = torch.device("cuda", 0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS * 1e3          # us per call


def ab(routes):
    """{name: fn} -> {name: (median, min, max)} us, the routes alternating run by run."""
    for fn in routes.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in routes}
    for _ in range(REPEATS):
        for k, fn in routes.items():
            runs[k].append(timed(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in runs.items()}


def fmt(r):
    return f"{r[0]:9.1f} us ({r[1]:.1f} - {r[2]:.1f})"


def route(own, gemm=None):
    xattn_hip.OWN = own
    if gemm is not None:
        vit_ops.OWN_GEMM = gemm


def cross_attention():
    B, H, d, L, Dc = 32, 8, 64, 64, 1024
    g = torch.Generator().manual_seed(0)
    module = CrossAttention(dim=H * d, dim_context=Dc, dim_head=d, heads=H)
    with torch.no_grad():                            # to_out is zero-initialised: give the backward real gradients
        module.to_out.weight.copy_(torch.randn(module.to_out.weight.shape, generator=g) * 0.02)
    module = module.to(DEV)
    context = torch.randn(B, L, Dc, generator=g).to(DEV)
    lengths = torch.randint(4, L + 1, (B,), generator=g)
    mask = (torch.arange(L)[None] < lengths[:, None]).to(DEV)
    say(f"CrossAttention fwd + bwd, B {B}, {H} heads of {d}, {L} text tokens of width {Dc}, padding mask "
        f"(lengths {int(lengths.min())}..{int(lengths.max())})")
    for side in (8, 16, 32):
        fmap = torch.randn(B, H * d, side, side, generator=g).to(DEV).requires_grad_(True)
        dy = torch.randn(B, H * d, side, side, generator=g).to(DEV)

        def step(own):
            route(own)
            y = module(fmap, context, mask=mask)
            torch.autograd.grad(y, [fmap] + list(module.parameters()), dy)

        r = ab({"hip": lambda: step("hip"), "torch": lambda: step("torch")})
        say(f"  Nq {side * side:5d}: hip {fmt(r['hip'])} | torch {fmt(r['torch'])} | torch / hip "
            f"{r['torch'][0] / r['hip'][0]:.2f}x")
    route("hip")


def text_tower():
    B = 32
    cfg = siglip_text_config_from_name("google/siglip2-large-patch16-512")
    tower = SiglipTextModel(cfg)
    tower.reset_parameters()
    tower = tower.eval().requires_grad_(False).to(DEV)
    texts = ["a photo of a %s" % ("very " * (i % 9) + "small cat") for i in range(B)]
    tok = ByteTokenizer()(texts)
    ids, mask = tok["input_ids"].to(DEV), tok["attention_mask"].to(DEV)
    say(f"SigLIP2-large text tower ({cfg.num_hidden_layers} layers, hidden {cfg.hidden_size}), B {B}, bf16, "
        f"lengths {int(mask.sum(1).min())}..{int(mask.sum(1).max())}")

    def run(own, gemm):
        route(own, gemm)
        tower(ids, mask, compute_dtype=torch.bfloat16)

    r = ab({"hip": lambda: run("hip", True), "torch": lambda: run("torch", False),
            "attn": lambda: run("hip", False), "gemm": lambda: run("torch", True)})
    say(f"  tower   : hip {fmt(r['hip'])} | torch {fmt(r['torch'])} | torch / hip {r['torch'][0] / r['hip'][0]:.2f}x")
    say(f"  mixed   : own attention + hipBLASLt GEMMs {fmt(r['attn'])} | SDPA + own GEMMs {fmt(r['gemm'])}")
    route("hip", True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    say(f"median of {REPEATS} runs of {ITERS} calls (min - max of the runs), {torch.cuda.get_device_name(0)}")
    cross_attention()
    text_tower()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
