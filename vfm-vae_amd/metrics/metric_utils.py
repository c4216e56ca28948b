"""Shared machinery of the quality metrics, with the reference's names (metrics/metric_utils.py) so configs
and callers carry over: MetricOptions, ProgressMonitor, FeatureStats, get_feature_detector and the two
feature sweeps.

What differs from the reference, and why:
  * FeatureStats.append_torch keeps raw_mean / raw_cov and the captured features on the device for ROCm
    batches and updates them with torch_utils.ops.fidstats_hip.accumulate (fp64 MFMA, no host sync per batch);
    the reference copies every batch to the host and multiplies there (:109-136). get_mean_cov reads the
    sums back once.
  * get_feature_detector never opens a URL: the file name of `url` is looked up in VFM_DETECTOR_DIR, else
    dnnlib.make_cache_dir_path('detectors'); a missing file is a FileNotFoundError naming the path.
  * compute_feature_stats_for_generator: the "generated" images are the autoencoder's reconstructions
    G(real, c, validation=True).gen_img of the same dataset items (rFID), not samples of a StyleGAN-T mapping /
    synthesis pair, which this generator does not have.
  * any dataset class works: map-style (`__getitem__`, through a DataLoader over this rank's items) or the
    training loop's streams (`iterate(batch_size, rank, world, seed)`).
"""
import hashlib
import os
import pickle
import random
import time
import uuid
from pathlib import Path

import numpy as np
import torch

import dnnlib
from torch_utils.ops import fidstats_hip


class MetricOptions:
    def __init__(self, G=None, G_kwargs={}, dataset_kwargs={}, num_gpus=1, rank=0, device=None, cache=True,
                 progress=None):
        if not 0 <= rank < num_gpus:
            raise ValueError(f"rank {rank} outside 0 .. {num_gpus - 1}")
        self.G = G
        self.G_kwargs = dnnlib.EasyDict(G_kwargs)
        self.dataset_kwargs = dnnlib.EasyDict(dataset_kwargs)
        self.num_gpus = num_gpus
        self.rank = rank
        self.device = device if device is not None else torch.device('cuda')
        self.progress = progress.sub() if progress is not None and rank == 0 else ProgressMonitor()
        self.cache = cache


def format_time(seconds):
    s = int(round(seconds))
    if s < 60:
        return f"{s}s"
    if s < 3600:
        return f"{s // 60}m {s % 60:02d}s"
    if s < 86400:
        return f"{s // 3600}h {s // 60 % 60:02d}m {s % 60:02d}s"
    return f"{s // 86400}d {s // 3600 % 24:02d}h {s // 60 % 60:02d}m"


class ProgressMonitor:
    def __init__(self, tag=None, num_items=None, flush_interval=1000, verbose=False, progress_fn=None, pfn_lo=0,
                 pfn_hi=1000, pfn_total=1000):
        self.tag = tag
        self.num_items = num_items
        self.verbose = verbose
        self.flush_interval = flush_interval
        self.progress_fn = progress_fn
        self.pfn_lo = pfn_lo
        self.pfn_hi = pfn_hi
        self.pfn_total = pfn_total
        self.start_time = time.time()
        self.batch_time = self.start_time
        self.batch_items = 0
        if progress_fn is not None:
            progress_fn(pfn_lo, pfn_total)

    def update(self, cur_items):
        assert self.num_items is None or cur_items <= self.num_items
        last = self.num_items is not None and cur_items >= self.num_items
        if cur_items < self.batch_items + self.flush_interval and not last:
            return
        now = time.time()
        if self.verbose and self.tag is not None:
            per_item = (now - self.batch_time) / max(cur_items - self.batch_items, 1)
            print(f"[{self.tag}] {cur_items} items in {format_time(now - self.start_time)}, "
                  f"{per_item * 1e3:.2f} ms per item", flush=True)
        self.batch_time = now
        self.batch_items = cur_items
        if self.progress_fn is not None and self.num_items is not None:
            self.progress_fn(self.pfn_lo + (self.pfn_hi - self.pfn_lo) * (cur_items / self.num_items), self.pfn_total)

    def sub(self, tag=None, num_items=None, flush_interval=1000, rel_lo=0, rel_hi=1):
        span = self.pfn_hi - self.pfn_lo
        return ProgressMonitor(tag=tag, num_items=num_items, flush_interval=flush_interval, verbose=self.verbose,
                               progress_fn=self.progress_fn, pfn_lo=self.pfn_lo + span * rel_lo,
                               pfn_hi=self.pfn_lo + span * rel_hi, pfn_total=self.pfn_total)


# ---------------------------------------------------------------------------------------------- detectors

_feature_detector_cache = dict()
_DETECTOR_EXTS = ('.pkl', '.pt', '.ts')


def get_feature_detector_name(url):
    return os.path.splitext(url.split('/')[-1])[0]


def detector_dir():
    return os.environ.get('VFM_DETECTOR_DIR') or dnnlib.make_cache_dir_path('detectors')


def detector_path(url):
    """The local file that stands for `url`: <detector dir>/<file name of url>. If that file is absent, the same
    stem with another detector extension (.pkl / .pt / .ts) is taken; if none exists, the first path is returned
    (the one a FileNotFoundError names)."""
    name = url.split('/')[-1]
    want = os.path.join(detector_dir(), name)
    if os.path.isfile(want):
        return want
    stem = os.path.splitext(name)[0]
    for ext in _DETECTOR_EXTS:
        alt = os.path.join(detector_dir(), stem + ext)
        if os.path.isfile(alt):
            return alt
    return want


def load_detector_file(path):
    if not os.path.isfile(path):
        raise FileNotFoundError(f"feature detector not found: expected {path} (set VFM_DETECTOR_DIR to the folder "
                                "that holds it; detectors are never downloaded)")
    if path.endswith('.pkl'):
        with open(path, 'rb') as f:
            try:
                import dill
                return dill.load(f)
            except ImportError:
                return pickle.load(f)
    return torch.jit.load(path, map_location='cpu')


def get_feature_detector(url, device=torch.device('cpu'), num_gpus=1, rank=0, verbose=False):
    if not 0 <= rank < num_gpus:
        raise ValueError(f"rank {rank} outside 0 .. {num_gpus - 1}")
    key = (url, device)
    if key not in _feature_detector_cache:
        path = detector_path(url)
        if verbose and rank == 0:
            print(f"Loading feature detector {path}")
        detector = load_detector_file(path).eval().to(device)
        for p in detector.parameters():                # (a ScriptModule has no requires_grad_())
            p.requires_grad_(False)
        _feature_detector_cache[key] = detector
    return _feature_detector_cache[key]


# ------------------------------------------------------------------------------------------- FeatureStats

class FeatureStats:
    """Running feature statistics with the reference's fields. raw_mean / raw_cov / all_features live on the host
    (numpy) until a ROCm batch arrives through append_torch; from then on they live on that device (torch) and
    every batch, host or device, is accumulated there."""

    def __init__(self, capture_all=False, capture_mean_cov=False, max_items=None):
        self.capture_all = capture_all
        self.capture_mean_cov = capture_mean_cov
        self.max_items = max_items
        self.num_items = 0
        self.num_features = None
        self.all_features = None
        self.raw_mean = None
        self.raw_cov = None

    def _on_device(self):
        return torch.is_tensor(self.raw_mean)

    def set_num_features(self, num_features, device=None):
        if self.num_features is not None:
            assert num_features == self.num_features
        else:
            self.num_features = num_features
            self.all_features = []
            self.raw_mean = np.zeros([num_features], dtype=np.float64)
            self.raw_cov = np.zeros([num_features, num_features], dtype=np.float64)
        if device is not None and device.type == 'cuda' and not self._on_device():
            self.raw_mean = torch.from_numpy(self.raw_mean).to(device)
            self.raw_cov = torch.from_numpy(self.raw_cov).to(device)
            self.all_features = [torch.from_numpy(f).to(device) for f in self.all_features]

    def is_full(self):
        return self.max_items is not None and self.num_items >= self.max_items

    def _room(self, n):
        """How many of n new items still fit under max_items."""
        return n if self.max_items is None else max(0, min(n, self.max_items - self.num_items))

    def append(self, x):
        if self._on_device():
            return self._append_device(torch.as_tensor(np.asarray(x, dtype=np.float32)).to(self.raw_mean.device))
        x = np.asarray(x, dtype=np.float32)
        assert x.ndim == 2
        room = self._room(x.shape[0])
        if room < x.shape[0]:
            if room == 0:
                return
            x = x[:room]
        self.set_num_features(x.shape[1])
        self.num_items += x.shape[0]
        if self.capture_all:
            self.all_features.append(x)
        if self.capture_mean_cov:
            x64 = x.astype(np.float64)
            self.raw_mean += x64.sum(axis=0)
            self.raw_cov += x64.T @ x64

    def _append_device(self, x):
        assert x.ndim == 2
        room = self._room(x.shape[0])                 # max_items is host state: no sync
        if room < x.shape[0]:
            if room == 0:
                return
            x = x[:room]
        self.set_num_features(x.shape[1], device=x.device)
        self.num_items += x.shape[0]
        if self.capture_all:
            self.all_features.append(x.to(torch.float32))
        if self.capture_mean_cov:
            if x.dtype not in (torch.float32, torch.float16):
                x = x.to(torch.float32)
            fidstats_hip.accumulate(self.raw_mean, self.raw_cov, x)

    def append_torch(self, x, num_gpus=1, rank=0):
        assert isinstance(x, torch.Tensor) and x.ndim == 2
        assert 0 <= rank < num_gpus
        if num_gpus > 1:
            # sample i of rank r becomes item i * num_gpus + r, as the reference's broadcast-and-stack order
            parts = [torch.empty_like(x) for _ in range(num_gpus)]
            torch.distributed.all_gather(parts, x.contiguous())
            x = torch.stack(parts, dim=1).flatten(0, 1)
        if x.is_cuda or self._on_device():
            self._append_device(x if x.is_cuda else x.to(self.raw_mean.device))
        else:
            self.append(x.cpu().numpy())

    def get_all(self):
        assert self.capture_all
        if self._on_device():
            return torch.cat(self.all_features, dim=0).cpu().numpy()
        return np.concatenate(self.all_features, axis=0)

    def get_all_torch(self):
        """All captured features, on the device they were captured on."""
        assert self.capture_all
        if self._on_device():
            return torch.cat(self.all_features, dim=0)
        return torch.from_numpy(self.get_all())

    def get_mean_cov(self):
        assert self.capture_mean_cov
        raw_mean, raw_cov = self.raw_mean, self.raw_cov
        if self._on_device():                         # the one read-back
            raw_mean, raw_cov = raw_mean.cpu().numpy(), raw_cov.cpu().numpy()
        mean = raw_mean / self.num_items
        return mean, raw_cov / self.num_items - np.outer(mean, mean)      # E[x x^T] - E[x] E[x]^T

    def _host_dict(self):
        d = dict(self.__dict__)
        if self._on_device():
            d['raw_mean'] = self.raw_mean.cpu().numpy()
            d['raw_cov'] = self.raw_cov.cpu().numpy()
            d['all_features'] = [f.cpu().numpy() for f in self.all_features]
        return d

    def save(self, pkl_file):
        import dill
        with open(pkl_file, 'wb') as f:
            dill.dump(self._host_dict(), f)

    @staticmethod
    def load(pkl_file):
        import dill
        with open(pkl_file, 'rb') as f:
            s = dnnlib.EasyDict(dill.load(f))
        obj = FeatureStats(capture_all=s.capture_all, max_items=s.max_items)
        obj.__dict__.update(s)
        return obj


# --------------------------------------------------------------------------------------- dataset sweeps

def _rank_items(num_items, num_gpus, rank):
    return [(i * num_gpus + rank) % num_items for i in range((num_items - 1) // num_gpus + 1)]


def _as_uint8_batch(images):
    if not torch.is_tensor(images):
        images = torch.from_numpy(np.stack(images))
    return images


def iterate_dataset(opts, dataset, item_subset, batch_size, data_loader_kwargs=None):
    """(uint8 images [b, C, H, W], labels) batches of this rank's items. Map-style datasets are read at
    `item_subset` through a DataLoader; stream datasets (`iterate`) yield len(item_subset) items of this rank's
    stream."""
    if hasattr(dataset, '__getitem__'):
        if data_loader_kwargs is None:
            data_loader_kwargs = dict(pin_memory=opts.device.type == 'cuda', num_workers=3, prefetch_factor=2)
        loader = torch.utils.data.DataLoader(dataset=dataset, sampler=item_subset, batch_size=batch_size,
                                             **data_loader_kwargs)
        for images, labels in loader:
            yield _as_uint8_batch(images), labels
        return
    if not hasattr(dataset, 'iterate'):
        raise TypeError(f"{type(dataset).__name__} has neither __getitem__ nor iterate(): the metrics cannot read it")
    left = len(item_subset)
    stream = dataset.iterate(batch_size=batch_size, rank=opts.rank, world=opts.num_gpus, seed=0)
    try:
        while left > 0:
            images, labels = next(stream)
            images = _as_uint8_batch(images)[:left]
            yield images, labels[:images.shape[0]]
            left -= images.shape[0]
    finally:
        getattr(stream, 'close', lambda: None)()


def _features(detector, images, detector_kwargs, device):
    if images.shape[1] == 1:
        images = images.repeat([1, 3, 1, 1])
    with torch.no_grad():
        return detector(images.to(device), **detector_kwargs)


def _dataset_cache_file(opts, detector_url, detector_kwargs, stats_kwargs, shuffle_size):
    args = dict(dataset_kwargs=opts.dataset_kwargs, detector_url=detector_url, detector_kwargs=detector_kwargs,
                stats_kwargs=stats_kwargs, shuffle_size=shuffle_size)
    digest = hashlib.md5(repr(sorted(args.items())).encode('utf-8')).hexdigest()
    tag = f"{Path(opts.dataset_kwargs.path).stem}-{get_feature_detector_name(detector_url)}-{digest}"
    return dnnlib.make_cache_dir_path('gan-metrics', tag + '.pkl')


def compute_feature_stats_for_dataset(opts, detector_url, detector_kwargs={}, rel_lo=0, rel_hi=1, batch_size=64,
                                      data_loader_kwargs=None, max_items=None, shuffle_size=None, **stats_kwargs):
    cache_file = None
    if opts.cache and 'path' in opts.dataset_kwargs:
        cache_file = _dataset_cache_file(opts, detector_url, detector_kwargs, stats_kwargs, shuffle_size)
        found = os.path.isfile(cache_file) if opts.rank == 0 else False
        if opts.num_gpus > 1:                          # every rank takes rank 0's answer
            flag = torch.as_tensor(float(found), dtype=torch.float32, device=opts.device)
            torch.distributed.broadcast(tensor=flag, src=0)
            found = float(flag.cpu()) != 0
        if found:
            return FeatureStats.load(cache_file)

    dataset = dnnlib.util.construct_class_by_name(**opts.dataset_kwargs)
    num_items = len(dataset)
    if max_items is not None:
        num_items = min(num_items, max_items)
    stats = FeatureStats(max_items=num_items, **stats_kwargs)
    progress = opts.progress.sub(tag='dataset features', num_items=num_items, rel_lo=rel_lo, rel_hi=rel_hi)
    detector = get_feature_detector(url=detector_url, device=opts.device, num_gpus=opts.num_gpus, rank=opts.rank,
                                    verbose=progress.verbose)
    item_subset = _rank_items(num_items, opts.num_gpus, opts.rank)
    if shuffle_size is not None:
        random.shuffle(item_subset)
        item_subset = item_subset[:shuffle_size]
    for images, _labels in iterate_dataset(opts, dataset, item_subset, batch_size, data_loader_kwargs):
        stats.append_torch(_features(detector, images, detector_kwargs, opts.device), num_gpus=opts.num_gpus,
                           rank=opts.rank)
        progress.update(stats.num_items)

    if cache_file is not None and opts.rank == 0:
        os.makedirs(os.path.dirname(cache_file), exist_ok=True)
        temp_file = cache_file + '.' + uuid.uuid4().hex
        stats.save(temp_file)
        os.replace(temp_file, cache_file)              # atomic
    return stats


def reconstruct_uint8(G, images, labels, device):
    """uint8 reconstructions of a uint8 batch: G(real / 255, c, validation=True).gen_img from [-1, 1]."""
    real = images.to(device).to(torch.float32) / 255.
    c = labels if (isinstance(labels, (list, tuple)) and len(labels) and isinstance(labels[0], str)) else \
        (labels.to(device) if torch.is_tensor(labels) else labels)
    out = G(real, c, validation=True)
    img = out.gen_img if hasattr(out, 'gen_img') else out[0]
    return (img.to(torch.float32) * 127.5 + 128).clamp(0, 255).to(torch.uint8)


def compute_feature_stats_for_generator(opts, detector_url, detector_kwargs, rel_lo=0, rel_hi=1, batch_size=64,
                                        batch_gen=None, data_loader_kwargs=None, **stats_kwargs):
    """Features of the reconstructions of the first max_items dataset items (this rank's share of them), in the
    item order of compute_feature_stats_for_dataset. `batch_gen` is accepted for the reference's callers; the
    autoencoder runs whole batches."""
    import copy
    G = copy.deepcopy(opts.G).eval().requires_grad_(False).to(opts.device)
    dataset = dnnlib.util.construct_class_by_name(**opts.dataset_kwargs)
    stats = FeatureStats(**stats_kwargs)
    assert stats.max_items is not None
    stats.max_items = min(stats.max_items, len(dataset))
    progress = opts.progress.sub(tag='generator features', num_items=stats.max_items, rel_lo=rel_lo, rel_hi=rel_hi)
    detector = get_feature_detector(url=detector_url, device=opts.device, num_gpus=opts.num_gpus, rank=opts.rank,
                                    verbose=progress.verbose)
    item_subset = _rank_items(stats.max_items, opts.num_gpus, opts.rank)
    for images, labels in iterate_dataset(opts, dataset, item_subset, batch_size, data_loader_kwargs):
        with torch.no_grad():
            recon = reconstruct_uint8(G, images, labels, opts.device)
        stats.append_torch(_features(detector, recon, detector_kwargs, opts.device), num_gpus=opts.num_gpus,
                           rank=opts.rank)
        progress.update(stats.num_items)
    return stats
