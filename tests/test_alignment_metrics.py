"""Alignment analysis on the CPU: tools/evaluate_alignment/metrics.py (the torch path of
torch_utils/ops/knn_hip.py) against values the reference produced (tests/golden/alignment_golden.npz, written
by tests/golden/make_golden_alignment.py), its error cases and CLI, the kernels' C ABI argument checks, and
the feature extractor on a tiny generator. Tolerances: alignment_cases.py. No GPU needed."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import alignment_cases as ac
import net_cases
from conftest import PKG

TOOLS = os.path.join(PKG, "tools")


def _load(rel):
    path = os.path.join(TOOLS, rel)
    spec = importlib.util.spec_from_file_location(os.path.basename(rel)[:-3] + "_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def metrics():
    return _load("evaluate_alignment/metrics.py")


@pytest.mark.parametrize("case", ac.GAP_SAFE, ids=lambda c: ac.tag(*c))
def test_metrics_match_reference_golden(metrics, case):
    n, d, k, seed = case
    g = ac.golden_case(*case)
    a, b = ac.make_features(n, d, seed)
    assert torch.equal(a, g["A"]) and torch.equal(b, g["B"])               # the recipe is the golden's input
    assert min(ac.min_boundary_gap(a, k), ac.min_boundary_gap(b, k)) >= 10 * ac.tol(d)
    M = metrics.AlignmentMetrics
    got = M.cknna(a, b, topk=k)
    print(f"cknna {got!r} golden fp64 {g['cknna64']!r} fp32 {g['cknna32']!r} bound {ac.cknna_tol(d):.3e}")
    assert abs(g["cknna32"] - g["cknna64"]) <= 5e-8
    assert abs(got - g["cknna64"]) <= ac.cknna_tol(d)
    assert M.measure("cknna", a, b, topk=k) == got
    assert abs(M.mutual_knn(a, b, topk=k) - g["mutual_knn"]) <= 1e-6
    assert abs(M.cycle_knn(a, b, topk=k) - g["cycle_knn"]) <= 1e-6


def test_sparse_terms_equal_dense_formula_fp64():
    """The sums over the neighbour lists reproduce the dense fp64 formula on fp64 features."""
    from torch_utils.ops import knn_hip
    n, d, k, seed = ac.GAP_SAFE[0]
    a, b = (x.double() for x in ac.make_features(n, d, seed))
    iK, vK = knn_hip.gram_topk(a, k)
    iL, vL = knn_hip.gram_topk(b, k)
    assert iK.dtype == torch.int32 and vK.dtype == torch.float64
    t = knn_hip.cknna_terms(iK, vK, iL, vL).tolist()
    m = n

    def hsic(c, s, p):
        return (c + s / ((m - 1) * (m - 2)) - 2 * p / (m - 2)) / (m * (m - 3))
    got = hsic(*t[0:3]) / (np.sqrt(hsic(*t[3:6]) * hsic(*t[6:9])) + 1e-6)
    assert abs(got - ac.dense_cknna64(a, b, iK, iL)) <= 1e-14


def test_torch_path_tie_rule_and_chunking(monkeypatch):
    from torch_utils.ops import knn_hip
    g = torch.Generator().manual_seed(0)
    f = torch.randint(-3, 4, (150, 16), generator=g).float()
    f[90] = f[5]
    ri, rv = ac.topk64(f, 12)
    idx, val = knn_hip.gram_topk(f, 12)
    assert torch.equal(idx.long(), ri) and torch.equal(val.double(), rv)
    assert 90 in idx[5].tolist() and 5 not in idx[5].tolist()
    monkeypatch.setattr(knn_hip, "_CHUNK_ELEMS", 150 * 7)                     # 7 rows at a time
    idx2, val2 = knn_hip.gram_topk(f, 12)
    assert torch.equal(idx, idx2) and torch.equal(val, val2)
    i0, v0 = knn_hip.gram_topk(f, 3, exclude_self=False)
    r0 = ac.topk64(f, 3, exclude_self=False)
    assert torch.equal(i0.long(), r0[0]) and torch.equal(v0.double(), r0[1])
    z = torch.zeros(6, 4)
    z[:, 0] = torch.tensor([0.0, -0.0, 0.0, -0.0, 0.0, -0.0])              # all scores +-0: -0.0 == 0.0
    assert knn_hip.gram_topk(z, 3)[0].tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2], [0, 1, 2]]
    with pytest.raises(ValueError):
        knn_hip.gram_topk(f, 150)
    with pytest.raises(ValueError):
        knn_hip.gram_topk(f, 0)


def test_preparation_pipeline_equals_golden(metrics, tmp_path):
    g = ac.golden()
    r1, r2 = ac.make_raw_pair()
    assert torch.equal(r1, torch.from_numpy(g["prep/raw1"])) and torch.equal(r2, torch.from_numpy(g["prep/raw2"]))
    paths = []
    for i, raw in enumerate((r1, r2)):
        p = tmp_path / f"f{i}.pt"
        names = [f"img{j:04d}" for j in range(raw.shape[0])]
        torch.save({"features": raw, "names": names, "transformations": [{"mode": "clean"}] * len(names)}, p)
        paths.append(str(p))
    fa, fb = metrics.load_and_process_features(*paths, device="cpu")
    assert torch.equal(fa, torch.from_numpy(g["prep/out1"])) and torch.equal(fb, torch.from_numpy(g["prep/out2"]))
    assert float(r1.abs().max()) > 100 and float(fa.abs().max()) < 1.0      # the outliers were clamped
    assert metrics.remove_outliers(r1, 1) is r1
    q = metrics.remove_outliers(r1, 0.9)                                     # the per-row quantile form
    assert float(q.abs().max()) == float(torch.quantile(r1.abs(), 0.9, dim=1).mean())
    bad = r1.clone()
    bad[0, 0] = float("nan")
    torch.save({"features": bad, "names": [], "transformations": []}, tmp_path / "bad.pt")
    with pytest.raises(ValueError, match="non-finite"):
        metrics.load_and_process_features(str(tmp_path / "bad.pt"), paths[1], device="cpu")


def test_cknna_error_cases(metrics):
    M = metrics.AlignmentMetrics
    a, b = ac.make_features(12, 8, 0)
    full = M.cknna(a, b)                                                     # topk=None: N - 1
    assert full == M.cknna(a, b, topk=11)
    for bad in (1, 0, -3):
        with pytest.raises(ValueError):
            M.cknna(a, b, topk=bad)
    with pytest.raises(ValueError):
        M.cknna(a[:3], b[:3], topk=2)
    with pytest.raises(ValueError):
        M.cknna(a, b, topk=12)                                               # more neighbours than other rows
    with pytest.raises(NotImplementedError, match="unbiased"):
        M.cknna(a, b, topk=3, unbiased=False)
    with pytest.raises(NotImplementedError, match="distance_agnostic"):
        M.cknna(a, b, topk=3, distance_agnostic=True)
    with pytest.raises(ValueError, match="Unrecognized"):
        M.measure("cka", a, b)
    assert M.SUPPORTED_METRICS == ["cknna"]


def test_cknna_is_nan_when_the_normalising_hsic_product_is_negative(metrics, monkeypatch):
    """The unbiased estimator may go negative for small N or k; the ratio is then undefined (the reference's
    torch.sqrt gives nan), not a math domain error."""
    import math
    from torch_utils.ops import knn_hip
    a, b = ac.make_features(12, 8, 0)
    real = knn_hip.cknna_terms

    def flipped(*lists):
        t = real(*lists).clone()
        t[3:6] = -t[3:6]                                                       # HSIC(K, K) < 0 < HSIC(L, L)
        return t
    monkeypatch.setattr(knn_hip, "cknna_terms", flipped)
    assert math.isnan(metrics.AlignmentMetrics.cknna(a, b, topk=3))


def test_cli_writes_reference_keys(metrics, tmp_path, capsys):
    a, b = ac.make_features(40, 16, 1)
    for name, f in (("a.pt", a), ("b.pt", b)):
        torch.save({"features": f * 3.0, "names": [], "transformations": []}, tmp_path / name)
    out = tmp_path / "res" / "out.pt"
    metrics.main(["--feat-path1", str(tmp_path / "a.pt"), "--feat-path2", str(tmp_path / "b.pt"), "--output", str(out),
                  "--trials", "2", "--device", "cpu", "--metrics", "cknna", "mutual_knn"])
    text = capsys.readouterr().out
    for line in ("Loading features from:", "Preparing features...", "Normalizing features...",
                 "Computing alignment metrics (2 trials each):", "Computing cknna...", "Summary of results:",
                 "Total time:"):
        assert line in text
    saved = torch.load(out, weights_only=False)
    assert set(saved) == {"results", "feat_file1", "feat_file2", "metrics_computed", "trials", "total_time"}
    assert saved["metrics_computed"] == ["cknna", "mutual_knn"] and saved["trials"] == 2
    r = saved["results"]["cknna"]
    assert set(r) == {"mean", "std", "scores", "mean_time"} and len(r["scores"]) == 2 and r["std"] == 0.0
    fa, fb = metrics.load_and_process_features(str(tmp_path / "a.pt"), str(tmp_path / "b.pt"), device="cpu")
    assert r["scores"][0] == metrics.AlignmentMetrics.cknna(fa, fb, topk=10)  # --topk defaults to 10
    out2 = tmp_path / "out2.pt"
    metrics.main(["--feat-path1", str(tmp_path / "a.pt"), "--feat-path2", str(tmp_path / "b.pt"), "--output", str(out2),
                  "--device", "cpu", "--topk", "4"])
    s2 = torch.load(out2, weights_only=False)
    assert s2["metrics_computed"] == ["cknna"] and s2["trials"] == 1
    assert s2["results"]["cknna"]["scores"][0] == metrics.AlignmentMetrics.cknna(fa, fb, topk=4)


def test_c_abi_argument_checks_and_workspace_query():
    import torch_utils.custom_ops as co
    lib = co.get_native()
    p = ctypes.c_void_p(16)
    ch = ctypes.c_int(-1)
    assert lib.vfm_gram_topk_ws(130, 10, 0, ctypes.byref(ch)) == 2 * 130 * 10 * 8 and ch.value == 2
    assert lib.vfm_gram_topk_ws(130, 10, 1, ctypes.byref(ch)) == 0 and ch.value == 1
    assert lib.vfm_gram_topk_ws(130, 10, 7, ctypes.byref(ch)) == 2 * 130 * 10 * 8 and ch.value == 2
    assert lib.vfm_gram_topk_ws(128, 10, 0, ctypes.byref(ch)) == 0 and ch.value == 1
    # splits = 0: the fewest splits that fill >= 0.9 of their rounds of 512 resident workgroups
    assert lib.vfm_gram_topk_ws(65536, 10, 0, ctypes.byref(ch)) == 0 and ch.value == 1     # 512 row blocks
    assert lib.vfm_gram_topk_ws(10000, 10, 0, ctypes.byref(ch)) == 6 * 10000 * 10 * 8 and ch.value == 6   # 79 x 6 = 474
    assert lib.vfm_gram_topk_ws(50000, 10, 0, ctypes.byref(ch)) == 5 * 50000 * 10 * 8 and ch.value == 5   # 391 x 5 = 1955
    assert lib.vfm_gram_topk_ws(4096, 10, 0, ctypes.byref(ch)) == 16 * 4096 * 10 * 8 and ch.value == 16   # 32 x 16 = 512
    assert lib.vfm_gram_topk_ws(1000, 10, 3, ctypes.byref(ch)) > 0 and ch.value == 3       # 8 tiles: 3 + 3 + 2
    assert lib.vfm_gram_topk_ws(1 << 20, 64, 100, ctypes.byref(ch)) == 64 * (1 << 20) * 64 * 8 and ch.value == 64
    assert lib.vfm_gram_topk_ws(0, 10, 0, None) == -2
    assert lib.vfm_gram_topk_ws(100, 65, 0, None) == -2
    assert lib.vfm_gram_topk_ws(100, 10, -1, None) == -2
    assert lib.vfm_gram_topk(None, 32, 100, 32, 10, 1, 0, p, p, p, None) == -2
    assert lib.vfm_gram_topk(p, 32, 100, 32, 10, 1, 0, None, p, p, None) == -2
    assert lib.vfm_gram_topk(p, 31, 100, 32, 10, 1, 0, p, p, p, None) == -2               # ld < D
    assert lib.vfm_gram_topk(p, 32, 100, 0, 10, 1, 0, p, p, p, None) == -2
    assert lib.vfm_gram_topk(p, 32, 100, 32, 0, 1, 0, p, p, p, None) == -2
    assert lib.vfm_gram_topk(p, 32, 10, 32, 10, 1, 0, p, p, p, None) == -2                # k > N - 1
    assert lib.vfm_gram_topk(p, 32, 300, 32, 10, 1, 2, p, p, None, None) == -2            # two splits, no workspace
    assert lib.vfm_gram_topk(p, 32, 100, 32, 65, 1, 0, p, p, p, None) == -1               # no kernel past k = 64
    assert lib.vfm_cknna_terms_ws(1000) == (4 * 1000 + 10 * 4) * 8
    assert lib.vfm_cknna_terms_ws(0) == -2
    assert lib.vfm_cknna_terms(p, p, p, None, 100, 10, p, p, None) == -2
    assert lib.vfm_cknna_terms(p, p, p, p, 100, 10, p, None, None) == -2
    assert lib.vfm_cknna_terms(p, p, p, p, 100, 0, p, p, None) == -2
    assert lib.vfm_cknna_terms(p, p, p, p, 100, 65, p, p, None) == -1


def test_supported_and_timer_names():
    from torch_utils.ops import kernel_timer, knn_hip
    f = torch.zeros(10, 4)
    assert not knn_hip.supported(f, 3)                                        # CPU tensor
    assert not knn_hip.force_ref()
    assert kernel_timer.roc_match(kernel_timer.rocprof_name("gram_topk<f32>"),
                                  "void (anonymous namespace)::gram_topk_kernel((anonymous namespace)::KnnArgs)")
    assert kernel_timer.roc_match(kernel_timer.rocprof_name("cknna_terms<f32>"), "(anonymous namespace)::cknna_rows()")


# ------------------------------------------------------------------ extractor

@pytest.fixture(scope="module")
def extractor_setup(tmp_path_factory):
    import yaml
    from PIL import Image
    root = tmp_path_factory.mktemp("align")
    vfm = root / net_cases.VFM_DIRNAME
    vfm.mkdir()
    json.dump(dict(net_cases.SIGLIP_CFG, layer_norm_eps=1e-6), open(vfm / "config.json", "w"))
    gkw = dict(net_cases.g_kwargs(str(vfm)), class_name="networks.generator.Generator")
    cfg = root / "tiny.yaml"
    yaml.safe_dump({"G_kwargs": gkw}, open(cfg, "w"))
    ext = _load("evaluate_alignment/vaes/extract_features_by_vfm_vae.py")
    common = ext.common
    torch.manual_seed(3)
    G = common.build_vae(str(cfg), 64, torch.device("cpu"))
    with torch.no_grad():
        for p in G.parameters():
            p.add_(torch.randn_like(p) * 0.02)
    ckpt = root / "snap.pth"
    torch.save({"G": {}, "D": {}, "G_ema": G.state_dict(), "training_set_kwargs": {}}, ckpt)
    data = root / "data"
    rng = np.random.default_rng(11)
    stems = ["b_two", "a_one", "c_three"]
    for sub, size in (("clean", 64), ("noise_0.100", 64), ("noise_0.050", 72), ("mask_0.25", 64)):
        (data / sub).mkdir(parents=True)
        for s in stems:
            Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(data / sub / f"{s}.png")
    json.dump({"c_three": {"scale": 0.75, "rotation": 90}, "a_one": {"scale": 1.0, "rotation": 0}},
              open(data / "equivariance_transforms.json", "w"))
    return dict(root=root, cfg=str(cfg), ckpt=str(ckpt), data=data, ext=ext, common=common, stems=sorted(stems))


def _vae(s, device="cpu"):
    common = s["common"]
    G = common.build_vae(s["cfg"], 64, torch.device(device))
    inc = common.load_vae_weights(G, s["ckpt"], torch.device(device), log=lambda *a: None)
    assert not inc.missing_keys and not inc.unexpected_keys
    return G


def test_extractor_clean_noise_mask(extractor_setup):
    s, ext = extractor_setup, extractor_setup["ext"]
    out = s["root"] / "feats"
    ext.main(["--input-dir", str(s["data"]), "--output-dir", str(out), "--output-prefix", "tiny", "--mode", "clean",
              "--vae-pth", s["ckpt"], "--use-config", s["cfg"], "--resolution", "64", "--batch-size-per-gpu", "2",
              "--device", "cpu"])
    got = torch.load(out / "tiny_clean.pt", weights_only=True)
    assert set(got) == {"features", "names", "transformations"}
    assert got["names"] == s["stems"] and got["transformations"] == [{"mode": "clean"}] * 3
    assert got["features"].dtype == torch.float32 and got["features"].shape[0] == 3
    # encode samples the posterior from the global CPU RNG (as the reference's does): compare the tool and the
    # direct path from the same seed, same batches (sorted names, two then one)
    G = _vae(s)
    rk = s["common"].Rank("cpu")
    torch.manual_seed(17)
    files = ext.extract_features(G, str(s["data"]), str(out), "seeded", "clean", 64, 2, rk, log=lambda *a: None)
    got = torch.load(files[0], weights_only=True)
    assert got["names"] == s["stems"]
    torch.manual_seed(17)
    exp = []
    for batch in (s["stems"][:2], s["stems"][2:]):
        x = torch.stack([torch.from_numpy(ext.load_rgb(str(s["data"] / "clean" / f"{n}.png"), 64)).permute(2, 0, 1)
                         for n in batch])
        with torch.no_grad():
            exp.append(G.encode(x, eq_scale_factor=1.0, is_eq_prior=False).mean([-2, -1]))
    assert torch.equal(got["features"], torch.cat(exp))
    files = ext.extract_features(G, str(s["data"]), str(out), "tiny", "noise", 64, 2, rk, log=lambda *a: None)
    assert [os.path.basename(f) for f in files] == ["tiny_noise_0.050.pt", "tiny_noise_0.100.pt"]
    nz = torch.load(files[0], weights_only=True)                              # 72-pixel images: resized to 64
    assert nz["names"] == s["stems"] and nz["transformations"][0] == {"mode": "noise", "noise_level": 0.05}
    assert nz["features"].shape == got["features"].shape
    files = ext.extract_features(G, str(s["data"]), str(out), "tiny", "mask", 64, 2, rk, log=lambda *a: None)
    assert [os.path.basename(f) for f in files] == ["tiny_mask_0.25.pt"]
    assert torch.load(files[0], weights_only=True)["transformations"][2] == {"mode": "mask", "mask_ratio": 0.25}


def test_extractor_equivariance_passes_scale_and_rotation(extractor_setup):
    s, ext = extractor_setup, extractor_setup["ext"]
    G = _vae(s)
    calls = []
    orig = G.encode

    def spy(img, *a, **kw):
        calls.append((img.clone(), kw))
        return orig(img, *a, **kw)
    G.encode = spy
    out = s["root"] / "feats_eq"
    torch.manual_seed(19)
    files = ext.extract_features(G, str(s["data"]), str(out), "tiny", "equivariance", 64, 2, s["common"].Rank("cpu"),
                                 log=lambda *a: None)
    got = torch.load(files[0], weights_only=True)
    assert os.path.basename(files[0]) == "tiny_equivariance.pt" and got["names"] == ["a_one", "c_three"]
    assert got["transformations"] == [{"scale": 1.0, "rotation": 0, "mode": "equivariance"},
                                      {"scale": 0.75, "rotation": 90, "mode": "equivariance"}]
    assert [c[1] for c in calls] == [{"eq_scale_factor": 1.0, "is_eq_prior": True},
                                     {"eq_scale_factor": 0.75, "is_eq_prior": True}]
    plain = torch.from_numpy(ext.load_rgb(str(s["data"] / "clean" / "c_three.png"), 64))
    assert torch.equal(calls[1][0][0], torch.rot90(plain, 1, (0, 1)).permute(2, 0, 1))
    torch.manual_seed(19)                                                     # same posterior noise as the tool's run
    with torch.no_grad():
        exp = [orig(img, **kw).mean([-2, -1])[0] for img, kw in calls]
    assert torch.equal(got["features"], torch.stack(exp))
    empty = s["root"] / "no_json"
    (empty / "clean").mkdir(parents=True)
    files = ext.extract_features(G, str(empty), str(out), "none", "equivariance", 64, 2, s["common"].Rank("cpu"),
                                 log=lambda *a: None)
    assert torch.load(files[0], weights_only=True)["features"].shape == (0, 512)
