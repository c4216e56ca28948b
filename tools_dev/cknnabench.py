"""Microbench: AlignmentMetrics.cknna (tools/evaluate_alignment/metrics.py) at topk = 10 on the kernels
(csrc/knn.hip: fused Gram + row top-k on the exact-fp32 MFMA, then the O(N k^2) sums) vs the dense torch
formulation on the same GPU -- the reference's expression restated below: two N x N Gram matrices, torch.topk
on clones, scattered N x N masks, hsic_unbiased with its N x N . N x N torch.mm three times, TF32 allowed as
the reference's CLI sets it. Normalised random features, N = 10 000 and 50 000 at D = 32 and 1152.
Per shape: both values, the kernels' time over ROUNDS rounds of ITERS calls between device events, the dense
formulation's time (one call at N = 50 000; an out-of-memory failure is recorded as such), and the Gram
region's own time by the dispatch-bound kernel timer (the top-k kernel plus its split merge) as TF/s against
the 157.3 TF fp32 MFMA peak."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vfm-vae_amd"), ROOT]
import torch

from torch_utils.ops import kernel_timer, knn_hip

ROUNDS, ITERS, WARM = 3, 5, 2
PEAK_TF = 157.3
TOPK = 10
DEV = torch.device("cuda", 0)
SHAPES = [(10000, 32), (10000, 1152), (50000, 32), (50000, 1152)]


def load_metrics():
    path = os.path.join(ROOT, "vfm-vae_amd", "tools", "evaluate_alignment", "metrics.py")
    spec = importlib.util.spec_from_file_location("alignment_metrics_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hsic_unbiased_dense(K, L):
    m = K.shape[0]
    Kt, Lt = K.clone().fill_diagonal_(0), L.clone().fill_diagonal_(0)
    h = torch.sum(Kt * Lt.T) + torch.sum(Kt) * torch.sum(Lt) / ((m - 1) * (m - 2)) - 2 * torch.sum(torch.mm(Kt, Lt)) / (m - 2)
    return h / (m * (m - 3))


def dense_cknna(fa, fb, topk):
    n = fa.shape[0]
    K, L = fa @ fa.T, fb @ fb.T

    def similarity(K, L):
        Kh, Lh = K.clone().fill_diagonal_(float("-inf")), L.clone().fill_diagonal_(float("-inf"))
        iK, iL = torch.topk(Kh, topk, dim=1)[1], torch.topk(Lh, topk, dim=1)[1]
        del Kh, Lh
        mask = torch.zeros(n, n, device=fa.device).scatter_(1, iK, 1) * torch.zeros(n, n, device=fa.device).scatter_(1, iL, 1)
        return hsic_unbiased_dense(mask * K, mask * L)

    kl, kk, ll = similarity(K, L), similarity(K, K), similarity(L, L)
    return kl.item() / (torch.sqrt(kk * ll) + 1e-6).item()


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, out


def main():
    if not torch.cuda.is_available():
        sys.exit("cknnabench needs the GPU: a CPU timing says nothing about it")
    M = load_metrics().AlignmentMetrics
    torch.backends.cuda.matmul.allow_tf32 = True                  # the reference CLI's setting, for the dense path
    print(f"{torch.cuda.get_device_name(0)}; cknna topk = {TOPK}; kernels: {ROUNDS} rounds of {ITERS} calls, ms per call")
    for N, D in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(N + D)
        fa = torch.nn.functional.normalize(torch.randn(N, D, generator=g, device=DEV), dim=-1)
        fb = torch.nn.functional.normalize(0.6 * fa + 0.8 * torch.nn.functional.normalize(
            torch.randn(N, D, generator=g, device=DEV), dim=-1), dim=-1)
        splits = knn_hip.gram_topk_workspace(N, TOPK)[1]
        for _ in range(WARM):
            M.cknna(fa, fb, topk=TOPK)
        ts, value = [], None
        for _ in range(ROUNDS):
            t, value = timed(lambda: M.cknna(fa, fb, topk=TOPK), ITERS)
            ts.append(t)
        med = sorted(ts)[len(ts) // 2]
        print(f"N={N} D={D} (splits {splits}):")
        print("  hip   " + " ".join(f"{v:9.2f}" for v in ts) + f"   median {med:9.2f} ms   cknna {value:.9f}")
        dense_iters = 3 if N <= 10000 else 1
        try:
            torch.cuda.reset_peak_memory_stats()
            dense_cknna(fa, fb, TOPK)                                # warm-up (library heuristics, allocator)
            td, dv = timed(lambda: dense_cknna(fa, fb, TOPK), dense_iters)
            peak = torch.cuda.max_memory_allocated() / 2 ** 30
            print(f"  dense {td:9.2f} ms ({dense_iters} call{'s' if dense_iters > 1 else ''}, peak {peak:.1f} GiB)   "
                  f"cknna {dv:.9f}   dense / hip = {td / med:.1f}x   |difference| {abs(dv - value):.2e}")
        except torch.OutOfMemoryError as err:
            print(f"  dense: out of memory ({str(err).splitlines()[0][:120]})")
        torch.cuda.empty_cache()
        kernel_timer.enable(True)
        kernel_timer.calibrate()
        for _ in range(ITERS):
            M.cknna(fa, fb, topk=TOPK)
        for name, v in sorted(kernel_timer.summary().items()):
            ms = v["total_ms"] / v["launches"]
            line = f"  {name:18s} {ms:9.3f} ms per call (kernel timer, {v['timed_launches']} calls)"
            if v["flops"]:
                tf = v["flops"] / v["total_ms"] / 1e9
                line += f", {v['flops'] / v['launches'] / 1e12:.3f} TFLOP -> {tf:6.1f} TF/s = {tf / PEAK_TF:.3f} of {PEAK_TF} TF"
            print(line)
        kernel_timer.enable(False)
        sys.stdout.flush()
        del fa, fb


if __name__ == "__main__":
    main()
