"""Improved precision and recall (Kynkaanniemi et al. 2019; reference metrics/precision_recall.py) on the fused
distance kernels: torch_utils.ops.prknn_hip.knn_radius gives every manifold point its (nhood_size + 1)-th
neighbour distance and manifold_hits tells which probes fall inside some point's ball, with no distance matrix
in memory and no distance on the host (the reference builds row_batch_size x col_batch_size cdist blocks,
copies each to the host and runs kthvalue / <= / any there). The only host read is the final mean."""
import torch

from torch_utils.ops import prknn_hip

from . import metric_utils

VGG16_URL = 'https://api.ngc.nvidia.com/v2/models/nvidia/research/stylegan3/versions/1/files/metrics/vgg16.pkl'


def _slice(n, num_gpus, rank):
    per = (n + num_gpus - 1) // num_gpus
    return min(rank * per, n), min((rank + 1) * per, n)


def _all_gather_rows(x, n, num_gpus):
    """The ranks' row slices (of _slice) joined into the [n] whole."""
    per = (n + num_gpus - 1) // num_gpus
    pad = torch.zeros([per], dtype=x.dtype, device=x.device)
    pad[:x.shape[0]] = x
    parts = [torch.empty_like(pad) for _ in range(num_gpus)]
    torch.distributed.all_gather(parts, pad)
    return torch.cat(parts)[:n]


def manifold_fraction(manifold, probes, nhood_size, num_gpus=1, rank=0):
    """The share of `probes` rows inside the k-NN balls of `manifold` (both fp16 [*, D] on one device)."""
    if num_gpus == 1:
        radii = prknn_hip.knn_radius(manifold, nhood_size)
        return float(prknn_hip.manifold_hits(probes, manifold, radii)[1])
    r0, r1 = _slice(manifold.shape[0], num_gpus, rank)
    radii = _all_gather_rows(prknn_hip.knn_radius(manifold, nhood_size, rows=(r0, r1)), manifold.shape[0], num_gpus)
    p0, p1 = _slice(probes.shape[0], num_gpus, rank)
    if p1 > p0:
        hits = prknn_hip.manifold_hits(probes[p0:p1], manifold, radii)[0].to(torch.uint8)
    else:
        hits = torch.zeros([0], dtype=torch.uint8, device=probes.device)
    return float(_all_gather_rows(hits, probes.shape[0], num_gpus).to(torch.float32).mean())


def compute_pr(opts, max_real, num_gen, nhood_size, row_batch_size=None, col_batch_size=None):
    """(precision, recall). row_batch_size / col_batch_size are the reference's block sizes: accepted and
    ignored, the fused kernels have no blocks to size."""
    detector_kwargs = dict(return_features=True)
    max_real = max_real // opts.num_gpus
    real = metric_utils.compute_feature_stats_for_dataset(
        opts=opts, detector_url=VGG16_URL, detector_kwargs=detector_kwargs, rel_lo=0, rel_hi=0, capture_all=True,
        max_items=None, shuffle_size=max_real).get_all_torch().to(torch.float16).to(opts.device)
    gen = metric_utils.compute_feature_stats_for_generator(
        opts=opts, detector_url=VGG16_URL, detector_kwargs=detector_kwargs, rel_lo=0, rel_hi=1, capture_all=True,
        max_items=num_gen).get_all_torch().to(torch.float16).to(opts.device)
    results = dict()
    for name, manifold, probes in (('precision', real, gen), ('recall', gen, real)):
        value = manifold_fraction(manifold, probes, nhood_size, opts.num_gpus, opts.rank)
        results[name] = value if opts.rank == 0 else float('nan')
    return results['precision'], results['recall']
