"""Microbench: the metric kernels against the reference formulation on the same machine.

accumulate (csrc/fidstats.hip) at D = 2048, batch 64 and 1024: raw_mean / raw_cov updated on the device, against
what the reference's FeatureStats.append does with a device batch -- `.cpu().numpy()`, widen, `x.T @ x` in fp64
on the host (as many BLAS threads as the process has).
compute_pr's two passes (csrc/prknn.hip: knn_radius + manifold_hits, both directions) at N = 10 000 and 50 000,
D = 4096 fp16, nhood 3, against the reference formulation restated below on the same GPU: 10 000 x 10 000
torch.cdist blocks of the .float() features, every block copied to the host, kthvalue / <= / any there (one
call).
Per kernel region (dispatch-bound kernel timer): ms per call and the fraction of the fp16 MFMA peak (2500 TF
dense) or of the fp64 peak (78.6 TF, vector = matrix on this part) reached."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vfm-vae_amd"), ROOT]
import numpy as np
import torch

from torch_utils.ops import fidstats_hip, kernel_timer, prknn_hip

ROUNDS, ITERS, WARM = 3, 5, 2
PEAK_F16_TF, PEAK_F64_TF = 2500.0, 78.6
DEV = torch.device("cuda", 0)
NHOOD, BLOCK = 3, 10000


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, out


def wall(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters, out


def regions(fn, peak):
    kernel_timer.enable(True)
    kernel_timer.calibrate()
    for _ in range(ITERS):
        fn()
    for name, v in sorted(kernel_timer.summary().items()):
        tf = v["flops"] / v["total_ms"] / 1e9
        print(f"  {name:26s} {v['total_ms'] / v['launches']:9.3f} ms per call (kernel timer, {v['timed_launches']} calls), "
              f"{v['flops'] / v['launches'] / 1e12:.4f} TFLOP -> {tf:7.1f} TF/s = {tf / peak:.3f} of {peak} TF")
    kernel_timer.enable(False)


def bench_accumulate(n, D=2048):
    g = torch.Generator(device=DEV).manual_seed(n)
    x = torch.randn(n, D, generator=g, device=DEV)
    mean = torch.zeros(D, dtype=torch.float64, device=DEV)
    cov = torch.zeros(D, D, dtype=torch.float64, device=DEV)
    hmean, hcov = np.zeros([D]), np.zeros([D, D])

    def host():
        nonlocal hmean, hcov
        x64 = x.cpu().numpy().astype(np.float64)
        hmean += x64.sum(axis=0)
        hcov += x64.T @ x64

    for _ in range(WARM):
        fidstats_hip.accumulate(mean, cov, x)
        host()
    ts = [timed(lambda: fidstats_hip.accumulate(mean, cov, x), ITERS)[0] for _ in range(ROUNDS)]
    th = [wall(host, ITERS)[0] for _ in range(ROUNDS)]
    med, medh = sorted(ts)[1], sorted(th)[1]
    print(f"accumulate n={n} D={D}:")
    print("  hip   " + " ".join(f"{v:9.3f}" for v in ts) + f"   median {med:9.3f} ms per batch")
    print("  host  " + " ".join(f"{v:9.3f}" for v in th) + f"   median {medh:9.3f} ms per batch "
          f"({torch.get_num_threads()} threads)   host / hip = {medh / med:.1f}x")
    regions(lambda: fidstats_hip.accumulate(mean, cov, x), PEAK_F64_TF)
    sys.stdout.flush()


def pr_kernels(real, gen):
    out = []
    for manifold, probes in ((real, gen), (gen, real)):
        radii = prknn_hip.knn_radius(manifold, NHOOD)
        out.append(prknn_hip.manifold_hits(probes, manifold, radii)[1])
    return float(out[0]), float(out[1])


def pr_dense(real, gen):
    """The reference's compute_pr arithmetic: cdist blocks on the GPU, everything else on the host."""
    def distances(rows, cols):
        return torch.cat([torch.cdist(rows.unsqueeze(0).float(), c.unsqueeze(0).float())[0].clone().cpu()
                          for c in cols.split(BLOCK)], dim=1)
    out = []
    for manifold, probes in ((real, gen), (gen, real)):
        kth = torch.cat([distances(b, manifold).to(torch.float32).kthvalue(NHOOD + 1).values.to(torch.float16)
                         for b in manifold.split(BLOCK)])
        pred = torch.cat([(distances(b, manifold) <= kth).any(dim=1) for b in probes.split(BLOCK)])
        out.append(float(pred.to(torch.float32).mean()))
    return out[0], out[1]


def bench_pr(N, D=4096):
    g = torch.Generator(device=DEV).manual_seed(N)
    real = torch.randn(N, D, generator=g, device=DEV).to(torch.float16)
    gen = (0.97 * torch.randn(N, D, generator=g, device=DEV) + 0.02).to(torch.float16)
    for _ in range(WARM):
        pr_kernels(real, gen)
    ts, value = [], None
    for _ in range(ROUNDS):
        t, value = timed(lambda: pr_kernels(real, gen), ITERS if N <= 10000 else 1)
        ts.append(t)
    med = sorted(ts)[1]
    print(f"compute_pr N={N} D={D} fp16 nhood {NHOOD}:")
    print("  hip   " + " ".join(f"{v:9.2f}" for v in ts) + f"   median {med:9.2f} ms   precision {value[0]:.6f} "
          f"recall {value[1]:.6f}")
    td, dv = wall(lambda: pr_dense(real, gen), 1)
    print(f"  dense {td:9.2f} ms (1 call)   precision {dv[0]:.6f} recall {dv[1]:.6f}   dense / hip = {td / med:.1f}x")
    regions(lambda: pr_kernels(real, gen), PEAK_F16_TF)
    sys.stdout.flush()


def main():
    if not torch.cuda.is_available():
        sys.exit("prbench needs the GPU: a CPU timing says nothing about it")
    print(f"{torch.cuda.get_device_name(0)}; kernels: {ROUNDS} rounds of {ITERS} calls, ms per call")
    for n in (64, 1024):
        bench_accumulate(n)
    for N in (10000, 50000):
        bench_pr(N)


if __name__ == "__main__":
    main()
