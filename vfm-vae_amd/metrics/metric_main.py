"""Metric registry and reporting with the reference's interface (metrics/metric_main.py): register_metric,
is_valid_metric, list_valid_metrics, calc_metric, report_metric. fid50k_full / fid10k_full / pr50k3_full are
computed here; cs10k and the COCO metrics are registered, so configs that name them parse, and raise
NotImplementedError (open_clip and the COCO set are not available to this build)."""
import json
import os
import time

import torch

import dnnlib

from . import frechet_inception_distance
from . import metric_utils
from . import precision_recall

_metric_dict = dict()      # name -> fn(opts) -> dict of results


def register_metric(fn):
    assert callable(fn)
    _metric_dict[fn.__name__] = fn
    return fn


def is_valid_metric(metric):
    return metric in _metric_dict


def list_valid_metrics():
    return list(_metric_dict.keys())


def detector_urls(metric):
    """The detector files `metric` needs (the training loop checks them before the first step)."""
    if not is_valid_metric(metric):
        raise ValueError(f"unknown metric {metric!r}; valid: {list_valid_metrics()}")
    if metric.startswith('fid'):
        return [frechet_inception_distance.INCEPTION_URL]
    if metric.startswith('pr'):
        return [precision_recall.VGG16_URL]
    return []


def calc_metric(metric, **kwargs):
    """kwargs: see metric_utils.MetricOptions."""
    if not is_valid_metric(metric):
        raise ValueError(f"unknown metric {metric!r}; valid: {list_valid_metrics()}")
    opts = metric_utils.MetricOptions(**kwargs)
    start_time = time.time()
    results = _metric_dict[metric](opts)
    total_time = time.time() - start_time
    for key, value in list(results.items()):           # every rank reports rank 0's numbers
        if opts.num_gpus > 1:
            value = torch.as_tensor(value, dtype=torch.float64, device=opts.device)
            torch.distributed.broadcast(tensor=value, src=0)
            value = float(value.cpu())
        results[key] = value
    return dnnlib.EasyDict(results=dnnlib.EasyDict(results), metric=metric, total_time=total_time,
                           total_time_str=metric_utils.format_time(total_time), num_gpus=opts.num_gpus)


def report_metric(result_dict, run_dir=None, snapshot_path=None):
    """Print the result as one JSON line and append it to <run_dir>/metric-<name>.jsonl."""
    metric = result_dict['metric']
    assert is_valid_metric(metric)
    rel_snapshot = None
    if run_dir is not None and snapshot_path is not None:
        rel_snapshot = os.path.relpath(snapshot_path, run_dir)
    line = json.dumps(dict(result_dict, snapshot_path=rel_snapshot, timestamp=time.time()), ensure_ascii=False)
    print(line)
    if run_dir is not None and os.path.isdir(run_dir):
        with open(os.path.join(run_dir, f'metric-{metric}.jsonl'), 'at', encoding='utf-8') as f:
            f.write(line + '\n')


def _full_dataset(opts):
    opts.dataset_kwargs.update(max_size=None, xflip=False)


@register_metric
def fid50k_full(opts):
    _full_dataset(opts)
    return dict(fid50k_full=frechet_inception_distance.compute_fid(opts, max_real=None, num_gen=50000))


@register_metric
def fid10k_full(opts):
    _full_dataset(opts)
    return dict(fid10k_full=frechet_inception_distance.compute_fid(opts, max_real=None, num_gen=10000))


@register_metric
def pr50k3_full(opts):
    _full_dataset(opts)
    precision, recall = precision_recall.compute_pr(opts, max_real=200000, num_gen=50000, nhood_size=3,
                                                    row_batch_size=10000, col_batch_size=10000)
    return dict(pr50k3_full_precision=precision, pr50k3_full_recall=recall)


def _unavailable(name, what):
    def fn(opts):
        raise NotImplementedError(f"metric {name}: {what} is not available to this build")
    fn.__name__ = name
    return register_metric(fn)


cs10k = _unavailable('cs10k', 'the CLIP score (open_clip)')
cs10k_coco = _unavailable('cs10k_coco', 'the CLIP score (open_clip) on the COCO validation set')
fid30k_coco64 = _unavailable('fid30k_coco64', 'the COCO validation set')
fid30k_coco256 = _unavailable('fid30k_coco256', 'the COCO validation set')
