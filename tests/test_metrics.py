"""The metrics package (vfm-vae_amd/metrics) on the CPU against the reference's own numbers
(tests/golden/metrics_golden.npz, written by tests/golden/make_golden_metrics.py from the reference's
FeatureStats, compute_pr and compute_fid): statistics, Frechet distance, precision / recall on the torch path,
detector lookup, the training loop's and the evaluate tool's wiring. Fixtures: tests/metrics_cases.py."""
import functools
import importlib.util
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import metrics_cases as mc
from conftest import PKG, ROOT


@functools.lru_cache(maxsize=None)
def _gold():
    return mc.golden()


def _mu():
    from metrics import metric_utils
    return metric_utils


@pytest.fixture
def detectors(tmp_path, monkeypatch):
    """Stand-in detector files in a fresh folder, a fresh cache folder, and an empty detector cache."""
    folder = mc.write_detectors(str(tmp_path / "detectors"))
    monkeypatch.setenv("VFM_DETECTOR_DIR", folder)
    monkeypatch.setenv("DNNLIB_CACHE_DIR", str(tmp_path / "cache"))
    _mu()._feature_detector_cache.clear()
    yield folder
    _mu()._feature_detector_cache.clear()


# ------------------------------------------------------------------------------------------ FeatureStats

def _appended(x, torch_path=False, **kw):
    s = _mu().FeatureStats(**kw)
    for part in mc.chunks(x):
        s.append_torch(torch.from_numpy(part)) if torch_path else s.append(part)
    return s


@pytest.mark.parametrize("torch_path", [False, True])
def test_feature_stats_integer_fixture_bit_equal(torch_path):
    s = _appended(mc.stats_fixture("int"), torch_path, capture_mean_cov=True)
    g = _gold()
    assert np.array_equal(s.raw_mean, g["stats/int/raw_mean"]) and np.array_equal(s.raw_cov, g["stats/int/raw_cov"])
    mean, cov = s.get_mean_cov()
    assert np.array_equal(mean, g["stats/int/mean"]) and np.array_equal(cov, g["stats/int/cov"])
    assert s.num_items == 200 and s.num_features == mc.STATS_D


def test_feature_stats_float_fixture_within_the_rounding_bound():
    x = mc.stats_fixture("float")
    s = _appended(x, capture_mean_cov=True)
    g = _gold()
    err = np.abs(s.raw_cov - g["stats/float/raw_cov"])
    print(f"max |raw_cov - reference| {err.max():.3e}, bound min {mc.cov_bound(x).min():.3e}")
    assert (err <= mc.cov_bound(x)).all()
    a = np.abs(x.astype(np.float64)).sum(axis=0)
    assert (np.abs(s.raw_mean - g["stats/float/raw_mean"]) <= 2 * x.shape[0] * 2.0 ** -53 * a).all()


def test_fidstats_accumulate_torch_path():
    """torch_utils.ops.fidstats_hip.accumulate on CPU tensors: the fp64 torch path, in place; shape and dtype
    errors."""
    from torch_utils.ops import fidstats_hip
    x = mc.stats_fixture("int")
    mean = torch.zeros(mc.STATS_D, dtype=torch.float64)
    cov = torch.zeros(mc.STATS_D, mc.STATS_D, dtype=torch.float64)
    for part in mc.chunks(x):
        fidstats_hip.accumulate(mean, cov, torch.from_numpy(part))
    fidstats_hip.accumulate(mean, cov, torch.zeros(0, mc.STATS_D))
    g = _gold()
    assert np.array_equal(mean.numpy(), g["stats/int/raw_mean"]) and np.array_equal(cov.numpy(), g["stats/int/raw_cov"])
    with pytest.raises(ValueError):
        fidstats_hip.accumulate(mean, cov[:, :5], torch.from_numpy(x))
    with pytest.raises(ValueError):
        fidstats_hip.accumulate(mean.float(), cov, torch.from_numpy(x))


def test_feature_stats_save_load_and_max_items(tmp_path):
    x = mc.stats_fixture("float")
    s = _appended(x, capture_all=True, capture_mean_cov=True, max_items=150)
    assert s.num_items == 150 and s.is_full()
    assert np.array_equal(s.get_all(), x[:150]) and torch.equal(s.get_all_torch(), torch.from_numpy(x[:150]))
    ref = _mu().FeatureStats(capture_mean_cov=True)
    for part in mc.chunks(x[:150], [1, 17, 64, 3, 50, 15]):        # the truncated chunk sequence
        ref.append(part)
    assert np.array_equal(s.raw_cov, ref.raw_cov)
    s.append(x[:5])                                                  # full: ignored
    assert s.num_items == 150
    path = str(tmp_path / "stats.pkl")
    s.save(path)
    t = _mu().FeatureStats.load(path)
    assert t.num_items == 150 and t.max_items == 150 and t.capture_all and t.capture_mean_cov
    assert np.array_equal(t.raw_mean, s.raw_mean) and np.array_equal(t.raw_cov, s.raw_cov)
    assert np.array_equal(t.get_all(), s.get_all())


# -------------------------------------------------------------------------------------------- two ranks

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _entry(fn, rank, world, port, q):
    for p in (PKG, ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    try:
        from torch_utils import distributed as dist
        dist.init(backend="gloo")
        q.put((rank, globals()[fn](rank, world)))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, "ERROR " + traceback.format_exc()))


def _spawn(fn, world=2):
    """tests/test_distributed.py's launch: CPU ranks over gloo, every GPU hidden from them."""
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_entry, args=(fn, r, world, port, q)) for r in range(world)]
    hide = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}
    saved = {k: os.environ.get(k) for k in hide}
    os.environ.update(hide)
    try:
        for p in procs:
            p.start()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    res = {}
    try:
        for _ in procs:
            r, out = q.get(timeout=300)
            res[r] = out
            if isinstance(out, str) and out.startswith("ERROR"):
                raise AssertionError(out)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    return res


def _two_rank_worker(rank, world):
    from metrics import metric_utils, precision_recall
    x = mc.stats_fixture("int")
    mine = torch.from_numpy(x[rank::world].copy())                  # rank r holds items r, r + world, ...
    s = metric_utils.FeatureStats(capture_all=True, capture_mean_cov=True)
    for part in (mine[:37], mine[37:]):
        s.append_torch(part, num_gpus=world, rank=rank)
    real, gen = mc.lattice(*mc.LATTICE[0])
    r16, g16 = torch.from_numpy(real).to(torch.float16), torch.from_numpy(gen).to(torch.float16)
    precision = precision_recall.manifold_fraction(r16, g16, mc.NHOOD, world, rank)
    recall = precision_recall.manifold_fraction(g16, r16, mc.NHOOD, world, rank)
    return dict(all=s.get_all(), raw_cov=s.raw_cov, n=s.num_items, precision=precision, recall=recall)


def test_two_ranks_interleave_and_row_slices():
    """num_gpus = 2 over gloo: append_torch interleaves the ranks' samples (item i of rank r is item 2 i + r), and
    precision / recall from per-rank row slices equal the single-process golden values."""
    res = _spawn("_two_rank_worker", 2)
    x = mc.stats_fixture("int")
    g = _gold()
    t = mc.tag(mc.LATTICE[0])
    for r in range(2):
        assert res[r]["n"] == 200 and np.array_equal(res[r]["all"], x)
        assert np.array_equal(res[r]["raw_cov"], g["stats/int/raw_cov"])
        assert res[r]["precision"] == float(g[f"{t}/precision"]) and res[r]["recall"] == float(g[f"{t}/recall"])


# --------------------------------------------------------------------------------------- Frechet distance

def test_frechet_distance_equals_the_reference():
    from metrics.frechet_inception_distance import frechet_distance
    g = _gold()
    got = frechet_distance(g["fid/mu_gen"], g["fid/sigma_gen"], g["fid/mu_real"], g["fid/sigma_real"])
    assert got == float(g["fid/fid7"])


def _opts(**kw):
    return dict(G=mc.StandInG(), dataset_kwargs=dict(class_name="metrics_cases.TinyImageDataset", path="tiny"),
                num_gpus=1, rank=0, device=torch.device("cpu"), **kw)


def test_compute_fid_end_to_end(detectors):
    """compute_fid over the stand-in detector file, the stand-in autoencoder and the tiny dataset, against the
    reference's compute_fid on the same features. Tolerance: ten times what the reference's own value moves when
    its batches are appended in 1 chunk instead of 7, the same kind of reordering as this sweep's batches of 64.
    Both reference values are 157.02480833557385: the stand-in features are integers scaled by 2^-8, so every
    fp64 sum and cross product is exact in any order, the reference's value moves by 0.0, and 10 x 0.0 allows
    nothing: the values must be equal. (With a square root on the features the reference moved by 4.16e-10,
    17.35304467701363 -> 17.353044677430123, and this test passed within 4.16e-9 on the host the golden file was
    written on but missed by 2.5e-5 on a host whose BLAS adds x.T @ x up in another order: the near-singular
    covariance of the stand-in's correlated features amplifies last-bit differences, so the fixture was made exact.)
    The second call reads the dataset statistics from the cache file and gives the same value."""
    from metrics import frechet_inception_distance as fid_mod
    g = _gold()
    fid7, fid1 = float(g["fid/fid7"]), float(g["fid/fid1"])
    tol = 10 * abs(fid7 - fid1)
    opts = _mu().MetricOptions(**_opts())
    got = fid_mod.compute_fid(opts, max_real=None, num_gen=mc.FID_ITEMS)
    print(f"fid {got!r} reference {fid7!r} diff {abs(got - fid7):.3e} (allowed {tol:.3e})")
    assert abs(got - fid7) <= tol
    cache = os.path.join(os.environ["DNNLIB_CACHE_DIR"], "gan-metrics")
    assert len(os.listdir(cache)) == 1 and os.listdir(cache)[0].startswith("tiny-inception-2015-12-05-")
    assert fid_mod.compute_fid(_mu().MetricOptions(**_opts()), max_real=None, num_gen=mc.FID_ITEMS) == got


def test_calc_and_report_metric(detectors, tmp_path):
    from metrics import metric_main
    assert {"fid50k_full", "fid10k_full", "pr50k3_full", "cs10k"} <= set(metric_main.list_valid_metrics())
    assert metric_main.is_valid_metric("fid10k_full") and not metric_main.is_valid_metric("is50k")
    res = metric_main.calc_metric("fid10k_full", **_opts())
    assert abs(res.results.fid10k_full - float(_gold()["fid/fid7"])) <= 10 * abs(
        float(_gold()["fid/fid7"]) - float(_gold()["fid/fid1"]))
    assert res.metric == "fid10k_full" and res.num_gpus == 1
    metric_main.report_metric(res, run_dir=str(tmp_path), snapshot_path=str(tmp_path / "network-snapshot-00000001.pth"))
    line = json.loads(open(tmp_path / "metric-fid10k_full.jsonl").read().strip())
    assert line["results"]["fid10k_full"] == res.results.fid10k_full
    assert line["snapshot_path"] == "network-snapshot-00000001.pth"
    pr = metric_main.calc_metric("pr50k3_full", **_opts())
    assert 0.0 <= pr.results.pr50k3_full_precision <= 1.0 and 0.0 <= pr.results.pr50k3_full_recall <= 1.0


# -------------------------------------------------------------------------------------- precision / recall

@pytest.mark.parametrize("case", mc.LATTICE, ids=mc.tag)
def test_compute_pr_torch_path_equals_the_reference(case, monkeypatch):
    from metrics import precision_recall
    from torch_utils.ops import prknn_hip
    real, gen = mc.lattice(*case)
    g, t = _gold(), mc.tag(case)

    def stats(x):
        s = _mu().FeatureStats(capture_all=True)
        s.append(x)
        return s
    monkeypatch.setattr(_mu(), "compute_feature_stats_for_dataset", lambda **kw: stats(real))
    monkeypatch.setattr(_mu(), "compute_feature_stats_for_generator", lambda **kw: stats(gen))
    opts = _mu().MetricOptions(num_gpus=1, rank=0, device=torch.device("cpu"))
    precision, recall = precision_recall.compute_pr(opts, max_real=case[0], num_gen=case[1], nhood_size=mc.NHOOD,
                                                    row_batch_size=10000, col_batch_size=10000)
    assert precision == float(g[f"{t}/precision"]) and recall == float(g[f"{t}/recall"])
    r16, g16 = torch.from_numpy(real).to(torch.float16), torch.from_numpy(gen).to(torch.float16)
    for name, manifold, probes in (("precision", r16, g16), ("recall", g16, r16)):
        radii = prknn_hip.knn_radius(manifold, mc.NHOOD)
        assert radii.dtype == torch.float16 and np.array_equal(radii.numpy(), g[f"{t}/{name}/radii"])
        hits, mean = prknn_hip.manifold_hits(probes, manifold, radii)
        assert np.array_equal(hits.numpy(), g[f"{t}/{name}/pred"]) and float(mean) == float(g[f"{t}/{name}"])
    # small row chunks of the torch path give the same answer
    monkeypatch.setattr(prknn_hip, "_CHUNK_ELEMS", 7 * case[0])
    assert torch.equal(prknn_hip.knn_radius(r16, mc.NHOOD), torch.from_numpy(g[f"{t}/precision/radii"]))
    assert torch.equal(prknn_hip.knn_radius(r16, mc.NHOOD, rows=(5, 40)),
                       torch.from_numpy(g[f"{t}/precision/radii"])[5:40])


# ------------------------------------------------------------------------------------------ error cases

def test_error_cases(tmp_path, monkeypatch):
    from metrics import metric_main
    from torch_utils.ops import prknn_hip
    f = torch.zeros(4, 8, dtype=torch.float16)
    with pytest.raises(ValueError):
        prknn_hip.knn_radius(f, 4)                                   # k + 1 > N
    assert prknn_hip.knn_radius(f, 3).shape == (4,)                  # N = k + 1 is legal
    with pytest.raises(ValueError):
        prknn_hip.manifold_hits(f, f[:, :4], torch.zeros(4, dtype=torch.float16))
    monkeypatch.setenv("VFM_DETECTOR_DIR", str(tmp_path / "nothing_here"))
    _mu()._feature_detector_cache.clear()
    url = "https://example.invalid/metrics/inception-2015-12-05.pkl"
    with pytest.raises(FileNotFoundError) as e:
        _mu().get_feature_detector(url)
    assert str(tmp_path / "nothing_here" / "inception-2015-12-05.pkl") in str(e.value)
    with pytest.raises(NotImplementedError):
        metric_main.calc_metric("cs10k", **_opts())
    with pytest.raises(ValueError):
        metric_main.calc_metric("no_such_metric", **_opts())


def test_native_entry_points_refuse_bad_arguments():
    """The C entry points return an error code before any device work (no GPU needed)."""
    import ctypes
    from torch_utils import custom_ops
    lib = custom_ops.get_native()
    p = ctypes.c_void_p(256)
    assert lib.vfm_knn_radius(p, 8, 4, 8, 4, 0, 4, 0, p, p, None) == -2          # k + 1 > N
    assert lib.vfm_knn_radius(p, 8, 100, 0, 3, 0, 100, 0, p, p, None) == -2      # D < 1
    assert lib.vfm_knn_radius(p, 8, 100, 8, 64, 0, 100, 0, p, p, None) == -1     # k + 1 > 64: no kernel
    assert lib.vfm_knn_radius(p, 8, 100, 8, 3, 90, 20, 0, p, p, None) == -2      # row slice past the end
    assert lib.vfm_knn_radius(p, 4, 100, 8, 3, 0, 100, 0, p, p, None) == -2      # ld < D
    assert lib.vfm_manifold_hits(p, 8, 0, p, 8, 10, 8, p, 0, p, p, p, None) == -2
    assert lib.vfm_feature_stats_accum(p, 0, 8, 4, 0, p, p, None) == -2          # D < 1
    assert lib.vfm_feature_stats_accum(p, 3, 8, 4, 8, p, p, None) == -1          # fp64 input: no kernel
    chosen = ctypes.c_int(0)
    assert lib.vfm_knn_radius_ws(50000, 3, 50000, 0, ctypes.byref(chosen)) > 0 and 1 <= chosen.value <= 64
    assert lib.vfm_knn_radius_ws(10, 64, 10, 0, ctypes.byref(chosen)) == -2
    assert lib.vfm_manifold_hits_ws(300, 257, 5, ctypes.byref(chosen)) > 0 and chosen.value == 3


# ----------------------------------------------------------------------------------------------- callers

def _train_cfg(tmp_path, metrics):
    import net_cases
    from test_train_loop import _write_shards
    keys = _write_shards(str(tmp_path / "wds"), n_shards=2, per_shard=4)
    keep = tmp_path / "keep.json"
    json.dump(keys, open(keep, "w"))
    c2t = tmp_path / "c2t.json"
    json.dump({"0": "zero", "1": "one", "2": "two"}, open(c2t, "w"))
    vfm = tmp_path / net_cases.VFM_DIRNAME
    vfm.mkdir()
    json.dump(dict(net_cases.SIGLIP_CFG, layer_norm_eps=1e-6), open(vfm / "config.json", "w"))
    g_kw = dict(net_cases.g_kwargs(str(vfm)), class_name="networks.generator.Generator")
    for k in ("img_resolution", "conditional", "label_type"):
        g_kw.pop(k)
    cfg = dict(
        run_dir=str(tmp_path / "run"), random_seed=3,
        training_set_kwargs=dict(class_name="training.data_wds.WdsWrapper", path=str(tmp_path / "wds"), resolution=64,
                                 conditional=False, label_type="cls2text", data_augmentation=False, one_epoch=False,
                                 workers=1, sample_shuffle_size=2, filter_keys_path=str(keep),
                                 cls_to_text_path=str(c2t)),
        G_kwargs=g_kw,
        D_kwargs=dict(net_cases.D_KWARGS, class_name="networks.discriminator.ProjectedDiscriminator"),
        loss_kwargs=dict(net_cases.loss_kwargs(str(vfm)), class_name="training.loss.TotalLoss"),
        G_opt_kwargs=dict(class_name="torch.optim.Adam", lr=1e-4, betas=[0.0, 0.99], eps=1e-8),
        D_opt_kwargs=dict(class_name="torch.optim.Adam", lr=1e-4, betas=[0.0, 0.99], eps=1e-8),
        batch_size=2, accumulate_gradients=1, kimg_per_tick=0.002, image_snapshot_ticks=1, network_snapshot_ticks=1,
        total_kimg=0.004, ema_kimg=0.01, ema_rampup=0.05, metrics=metrics, cudnn_benchmark=False, resume_path=None,
        resume_kimg=0)
    for k in ("vfm_name", "resume_kimg"):
        cfg["loss_kwargs"].pop(k, None)
    return cfg


def test_training_loop_with_metrics(tmp_path, monkeypatch):
    """metrics=['fid10k_full']: without the detector file the loop raises before the first step (the message names
    the path); with a stand-in detector file a 2-tick run writes metric-fid10k_full.jsonl."""
    import yaml
    import train
    from training import training_loop as tl
    cfg = _train_cfg(tmp_path, ["fid10k_full"])
    cfg_path = tmp_path / "cfg.yaml"
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("DNNLIB_CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.setenv("VFM_DETECTOR_DIR", str(tmp_path / "no_detectors"))
    _mu()._feature_detector_cache.clear()
    steps = []
    orig = tl.TrainingIteration.__call__
    monkeypatch.setattr(tl.TrainingIteration, "__call__", lambda self, *a, **k: (steps.append(1), orig(self, *a, **k))[1])
    try:
        with pytest.raises(NotImplementedError) as e:
            train.main(["--config", str(cfg_path)])
        assert str(tmp_path / "no_detectors" / "inception-2015-12-05.pkl") in str(e.value) and steps == []
        torch.distributed.destroy_process_group() if torch.distributed.is_initialized() else None
        monkeypatch.setenv("VFM_DETECTOR_DIR", mc.write_detectors(str(tmp_path / "detectors")))
        train.main(["--config", str(cfg_path)])
    finally:
        torch.distributed.destroy_process_group() if torch.distributed.is_initialized() else None
        _mu()._feature_detector_cache.clear()
    assert steps
    lines = [json.loads(ln) for ln in open(tmp_path / "run" / "metric-fid10k_full.jsonl")]
    assert lines and np.isfinite(lines[-1]["results"]["fid10k_full"])
    assert lines[-1]["snapshot_path"].startswith("network-snapshot-")
    stats = [json.loads(ln) for ln in open(tmp_path / "run" / "stats.jsonl")]
    assert stats[-1]["Metrics/fid10k_full"] == lines[-1]["results"]["fid10k_full"]


def test_evaluate_tool_metrics_flags(detectors, tmp_path):
    """tools/reconstruct/evaluate.py --metrics fid pr on two tiny PNG folders with the stand-in detectors."""
    from PIL import Image
    path = os.path.join(PKG, "tools", "reconstruct", "evaluate.py")
    spec = importlib.util.spec_from_file_location("evaluate_tool_metrics", path)
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    a, b = tmp_path / "ref", tmp_path / "pred"
    a.mkdir()
    b.mkdir()
    ds = mc.TinyImageDataset(num_items=24)
    rng = np.random.default_rng(3)
    for i, img in enumerate(ds.images):
        hwc = img.transpose(1, 2, 0)
        Image.fromarray(hwc).save(a / f"{i:03d}.png")
        noisy = np.clip(hwc.astype(int) + rng.integers(-30, 31, hwc.shape), 0, 255).astype(np.uint8)
        Image.fromarray(noisy).save(b / f"{i:03d}.png")
    res = ev.evaluate_distribution_metrics(str(a), str(b), metrics=["fid", "pr"], detector_dir=detectors, nhood_size=3,
                                           batch_size=10, num_workers=2, device="cpu", log=lambda *x: None)
    assert res["total"] == 24 and np.isfinite(res["fid"]) and res["fid"] > 0
    assert 0.0 <= res["precision"] <= 1.0 and 0.0 <= res["recall"] <= 1.0
    same = ev.evaluate_distribution_metrics(str(a), str(a), metrics=["fid", "pr"], detector_dir=detectors,
                                            batch_size=24, num_workers=1, device="cpu", log=lambda *x: None)
    assert abs(same["fid"]) < 1e-6 and same["precision"] == 1.0 and same["recall"] == 1.0
    with pytest.raises(ValueError):
        ev.evaluate_distribution_metrics(str(a), str(b), metrics=["is"], detector_dir=detectors, device="cpu")
