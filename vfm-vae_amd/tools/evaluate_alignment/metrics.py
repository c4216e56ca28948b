"""Alignment metrics between two feature files (SE-CKNNA, mutual / cycle kNN).

Drop-in for the reference `tools/evaluate_alignment/metrics.py`: only its interface is kept -- the
`AlignmentMetrics` call signatures, the feature preparation entry points (`remove_outliers`,
`prepare_features`, `load_and_process_features`: exact 0.95 quantile clamp, then L2 normalisation), the CLI flags
(`--feat-path1 --feat-path2 --output --trials`), the printed lines and the keys of the saved dict. Two flags are
added, `--topk` (default 10, the value the reference hard-codes) and `--metrics`, plus `--device` as on the
other tools here (default: cuda when present, else cpu).

MI355X design: nothing here is N x N. The reference's `cknna` (:191-238) builds two dense Gram matrices, runs
torch.topk on clones of them, scatters three pairs of N x N masks and calls `hsic_unbiased` (:241-260) on the
masked copies with a full N x N . N x N torch.mm, three times, under TF32. After the top-k every matrix of
the formula has at most k non-zeros per row, so all of it follows from the two neighbour lists:

    sum(A o B^T) = sum_{(i,j), (j,i) in mask} A_ij B_ji      sum(A @ B) = sum_i sum_{j in mask(i)} A_ij rowsum(B)_j

`torch_utils.ops.knn_hip.gram_topk` produces the lists (fused Gram + row top-k on the exact-fp32 MFMA, the
score matrix never in memory) and `cknna_terms` the sums in fp64; the host combines nine numbers. Ties between
equal scores go to the lower index (torch.topk leaves them unspecified). `mutual_knn` and `cycle_knn` come
from the same lists with row-chunked [rows, k, k] tensor ops.

Differences from the reference, on purpose: `topk=None` means N - 1 (the reference compares None < 2 first and
raises TypeError); `topk < 2` or N < 4 raises ValueError (N <= 3 divides by zero in hsic_unbiased);
`unbiased=False` and `distance_agnostic=True` raise NotImplementedError (the CLI never uses the first; the
reference's own expression for the second returns a matrix and fails at `.item()`). Non-finite features are
refused on load. No torchaudio, sklearn or pymp.
"""
import math
import os
import sys
import time

PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_utils.ops import knn_hip  # noqa: E402

ALL_METRICS = ["cknna", "mutual_knn", "cycle_knn"]
_PAIR_ELEMS = 1 << 22          # elements of one [rows, k, k] chunk of the list-against-list comparisons


def _hsic_from_sums(cross, sums, product, m):
    """Unbiased HSIC (Song et al. 2012, eq. 5) of two zero-diagonal m x m matrices A, B from
    cross = sum(A o B^T), sums = sum(A) sum(B), product = sum(A @ B)."""
    return (cross + sums / ((m - 1) * (m - 2)) - 2.0 * product / (m - 2)) / (m * (m - 3))


def _neighbours(feats, k):
    """int64 [N, k]: each row's k nearest other rows by inner product (ties to the lower index)."""
    if feats.ndim != 2:
        raise ValueError(f"features must be [N, D], got {tuple(feats.shape)}")
    return knn_hip.gram_topk(feats, k, exclude_self=True)[0].long()


def _chunk_rows(k):
    return max(1, _PAIR_ELEMS // (k * k))


class AlignmentMetrics:
    SUPPORTED_METRICS = ["cknna"]

    @staticmethod
    def measure(metric, *args, **kwargs):
        """Call the supported metric named `metric` with the remaining arguments."""
        if metric in AlignmentMetrics.SUPPORTED_METRICS:
            return getattr(AlignmentMetrics, metric)(*args, **kwargs)
        raise ValueError(f"Unrecognized metric: {metric}")

    @staticmethod
    def cycle_knn(feats_A, feats_B, topk):
        """Fraction of rows i that are an A-neighbour of one of i's B-neighbours."""
        nn_a, nn_b = _neighbours(feats_A, topk), _neighbours(feats_B, topk)
        n, rows, found = nn_a.shape[0], _chunk_rows(topk), 0
        for r0 in range(0, n, rows):
            via = nn_a[nn_b[r0:r0 + rows]]                                    # [rows, k, k]
            me = torch.arange(r0, r0 + via.shape[0], device=via.device).view(-1, 1, 1)
            found += int((via == me).flatten(1).any(dim=1).sum())
        return found / n

    @staticmethod
    def mutual_knn(feats_A, feats_B, topk):
        """Mean over rows of |kNN_A(i) & kNN_B(i)| / topk."""
        nn_a, nn_b = _neighbours(feats_A, topk), _neighbours(feats_B, topk)
        shared = knn_hip.in_other(nn_a, nn_b, _chunk_rows(topk))
        return int(shared.sum()) / (nn_a.shape[0] * nn_a.shape[1])

    @staticmethod
    def cknna(feats_A, feats_B, topk=None, distance_agnostic=False, unbiased=True):
        """CKA restricted to mutual nearest neighbours: HSIC(M o K, M o L) / sqrt(HSIC(M_K o K, M_K o K)
        HSIC(M_L o L, M_L o L)), K / L the two Gram matrices, M_K / M_L their top-k masks, M = M_K o M_L.
        nan when the two normalising HSIC estimates have opposite signs (the unbiased estimator may go negative
        for small N or k), as the reference's sqrt gives."""
        n = feats_A.shape[0]
        if feats_B.shape[0] != n:
            raise ValueError(f"feature counts differ: {n} and {feats_B.shape[0]}")
        k = n - 1 if topk is None else int(topk)
        if k < 2:
            raise ValueError("CKNNA requires topk >= 2")
        if n < 4:
            raise ValueError("CKNNA requires at least 4 samples")
        if not unbiased:
            raise NotImplementedError("cknna(unbiased=False) (hsic_biased on dense masked Gram matrices) is not "
                                      "built; the alignment tool always runs unbiased=True")
        if distance_agnostic:
            raise NotImplementedError("cknna(distance_agnostic=True) is undefined in the reference as well (its "
                                      "expression yields a matrix)")
        idx_k, val_k = knn_hip.gram_topk(feats_A, k, exclude_self=True)
        idx_l, val_l = knn_hip.gram_topk(feats_B, k, exclude_self=True)
        t = knn_hip.cknna_terms(idx_k, val_k, idx_l, val_l).tolist()          # the one host sync
        kl, kk, ll = (_hsic_from_sums(*t[3 * h:3 * h + 3], n) for h in range(3))
        norm2 = kk * ll
        if not norm2 >= 0.0:
            return float("nan")
        return kl / (math.sqrt(norm2) + 1e-6)


def remove_outliers(feats, q, exact=False, max_threshold=None):
    """Clamp to +-t, t the q-quantile of |feats|: over the whole tensor by a sort when `exact` (element
    int(q numel) of the ascending order), else the mean of the per-row quantiles. q == 1 returns the input.
    `max_threshold` is accepted and, as in the reference, has no effect."""
    if q == 1:
        return feats
    mag = feats.abs()
    if exact:
        t = mag.reshape(-1).sort().values[int(q * feats.numel())]
    else:
        t = torch.quantile(mag.flatten(start_dim=1), q, dim=1).mean()
    return feats.clamp(-t, t)


def prepare_features(feats, q=0.95, exact=False, device=None):
    """fp32 features with their outliers clamped, on the compute device (cuda when present, else cpu)."""
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    return remove_outliers(feats.float(), q=q, exact=exact).to(device)


def load_and_process_features(feat_path1, feat_path2, device=None):
    """The 'features' of two extractor payloads (.pt), outliers clamped at the exact 0.95 quantile, rows
    L2-normalised. Non-finite features raise ValueError (checked once, here: the kernels do not order them)."""
    paths = (feat_path1, feat_path2)
    print("Loading features from:")
    for i, p in enumerate(paths, 1):
        print(f"  File {i}: {p}")
    raw = [torch.load(p, map_location="cpu", weights_only=True)["features"] for p in paths]
    print(f"Original feature shapes: {raw[0].shape}, {raw[1].shape}")
    for p, f in zip(paths, raw):
        if not bool(torch.isfinite(f).all()):
            raise ValueError(f"non-finite features in {p}")
    print("Preparing features...")
    clamped = [prepare_features(f, q=0.95, exact=True, device=device) for f in raw]
    print("Normalizing features...")
    return tuple(torch.nn.functional.normalize(f, dim=-1) for f in clamped)


def _run_trials(metric, feats_A, feats_B, trials, topk):
    fn = getattr(AlignmentMetrics, metric)
    scores, seconds = [], []
    for _ in range(trials):
        t0 = time.time()
        scores.append(fn(feats_A, feats_B, topk=topk))
        seconds.append(time.time() - t0)
    return {"mean": np.mean(scores), "std": np.std(scores), "scores": scores, "mean_time": np.mean(seconds)}


def compute_all_metrics(feats_A, feats_B, trials=10, topk=10, metrics=None):
    """{metric: {'mean', 'std', 'scores', 'mean_time'}} over `trials` calls of each metric (default: the
    supported ones) at `topk` neighbours."""
    names = list(AlignmentMetrics.SUPPORTED_METRICS) if metrics is None else list(metrics)
    unknown = [m for m in names if m not in ALL_METRICS]
    if unknown:
        raise ValueError(f"Unrecognized metric: {unknown[0]}")
    rule = "-" * 50
    print(f"\nComputing alignment metrics ({trials} trials each):")
    print(rule)
    results = {}
    for name in names:
        print(f"Computing {name}...")
        r = results[name] = _run_trials(name, feats_A, feats_B, trials, topk)
        print(f"{name.rjust(20)}: {r['mean']:.4f} ± {r['std']:.4f} [elapsed: {r['mean_time']:.3f}s]")
    print(rule)
    return results


def _parse_args(argv):
    import argparse
    p = argparse.ArgumentParser(description="Compute alignment metrics between two feature files")
    p.add_argument("--feat-path1", type=str, help="Path to first feature file (.pt)")
    p.add_argument("--feat-path2", type=str, help="Path to second feature file (.pt)")
    p.add_argument("--output", type=str, help="Optional output file to save results")
    p.add_argument("--trials", type=int, default=1, help="Number of trials for each metric")
    p.add_argument("--topk", type=int, default=10, help="Neighbours per sample")
    p.add_argument("--metrics", type=str, nargs="+", choices=ALL_METRICS,
                   default=list(AlignmentMetrics.SUPPORTED_METRICS), help="Metrics to compute")
    p.add_argument("--device", type=str, default=None, help="override (default cuda, else cpu)")
    return p.parse_args(argv)


def main(argv=None):
    args = _parse_args(argv)
    feats_A, feats_B = load_and_process_features(args.feat_path1, args.feat_path2, device=args.device)
    print(f"Final feature shapes: {feats_A.shape}, {feats_B.shape}")

    start = time.time()
    results = compute_all_metrics(feats_A, feats_B, trials=args.trials, topk=args.topk, metrics=args.metrics)
    total_time = time.time() - start

    if args.output:
        os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
        torch.save({"results": results, "feat_file1": args.feat_path1, "feat_file2": args.feat_path2,
                    "metrics_computed": list(args.metrics), "trials": args.trials, "total_time": total_time},
                   args.output)
        print(f"\nResults saved to: {args.output}")
    print("\nSummary of results:")
    for name, r in results.items():
        print(f"  {name}: {r['mean']:.4f} ± {r['std']:.4f}")
    print(f"\nTotal time: {total_time:.2f}s")
    return results


if __name__ == "__main__":
    main()
