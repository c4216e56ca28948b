"""Microbench: training.loss.SSIM on the HIP kernels (csrc/ssim.hip) vs the torch formulation of the same
commit (decoder_ops.set_force_ref(True): clamps, reflect pads, the 121-tap grouped convolution on MIOpen and
the elementwise chain), at the stage-2 step's shape (B = 32, 3 x 256^2, clamp, forward + backward to the
generated image) and at tools/reconstruct/evaluate.py's (B = 64, 3 x 256^2, no-grad forward).
The two paths alternate in one process over ROUNDS rounds of ITERS calls between device events, after a warm-up
of both; then the kernels' own times by the dispatch-bound kernel timer, with the algorithmic bytes over
them as a fraction of 8 TB/s."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vfm-vae_amd"), ROOT]
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
import torch

from training.loss import SSIM
from torch_utils.ops import decoder_ops, kernel_timer

ROUNDS, ITERS, WARM = 5, 50, 10
HBM_GBS = 8000.0
DEV = torch.device("cuda", 0)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    if not torch.cuda.is_available():
        sys.exit("ssimbench needs the GPU: a CPU timing says nothing about it")
    m = SSIM(data_range=2.0)
    g = torch.Generator(device=DEV).manual_seed(0)
    for label, B, grad in (("stage-2 step, fwd + bwd, clamp", 32, True), ("evaluate.py, no-grad fwd", 64, False)):
        real = (0.7 * torch.randn(B, 3, 256, 256, generator=g, device=DEV))
        gen = (real + 0.3 * torch.randn(B, 3, 256, 256, generator=g, device=DEV)).requires_grad_(grad)

        def call():
            if grad:
                gen.grad = None
                (1.0 - m(gen, real, clamp=(-1, 1))).backward()
                return gen.grad
            with torch.no_grad():
                return m(gen, real)

        def run(ref):
            decoder_ops.set_force_ref(ref)
            try:
                return call()
            finally:
                decoder_ops.set_force_ref(False)

        outs = {}
        for ref in (False, True):
            for _ in range(WARM):
                outs[ref] = run(ref).clone()
        torch.cuda.synchronize()
        d = (outs[False].double() - outs[True].double()).norm() / outs[True].double().norm()
        ts = {False: [], True: []}
        for _ in range(ROUNDS):
            for ref in (False, True):
                ts[ref].append(timed(lambda: run(ref), ITERS))
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        print(f"{label}: B={B} 3x256x256, {ROUNDS} alternating rounds of {ITERS} calls, us per call")
        print("  hip   " + " ".join(f"{v:8.1f}" for v in ts[False]) + f"   median {med[False]:8.1f}")
        print("  torch " + " ".join(f"{v:8.1f}" for v in ts[True]) + f"   median {med[True]:8.1f}")
        print(f"  torch / hip = {med[True] / med[False]:.2f}x; hip vs torch result, relative difference {float(d):.2e}")
        kernel_timer.enable(True)
        kernel_timer.calibrate()
        for _ in range(ITERS):
            run(False)
        for name, v in sorted(kernel_timer.summary().items()):
            us = v["total_ms"] * 1e3 / v["launches"]
            gbs = v["bytes"] / v["total_ms"] / 1e6
            print(f"  {name:14s} {us:7.1f} us per launch (kernel timer, {v['timed_launches']} launches), "
                  f"{v['bytes'] / v['launches'] / 1e6:.1f} MB algorithmic -> {gbs:7.1f} GB/s = {gbs / HBM_GBS:.3f} of 8 TB/s")
        kernel_timer.enable(False)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
