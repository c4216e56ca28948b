"""Fixtures shared by tests/test_metrics.py, tests/test_metrics_gpu.py and tests/golden/make_golden_metrics.py
(which feeds them to the reference's metrics package and records what it computes).

Lattice precision / recall fixture (exact on every path): C integer cluster centres in [-6, 6]^D; the real set
draws its centres from the first 3/4 of the clusters, the generated set from the last 3/4; integer noise in
{-1, 0, 1} on the first 8 dimensions only. All values are small integers (fp16-exact), squared distances are
integers below 2^24, so every summation order gives the same fp32 value, sqrtf is correctly rounded on both
sides, and a kernel has to reproduce the reference bit for bit -- including the many exact ties d == r and the
fp16 rounding of the radius.

Gaussian fixture (rounding matters): manifold randn, probes 0.97 randn + 0.02, cast to fp16. fp32 distances
differ from fp64 ones by at most band(a, b, d) = (D + 2) 2^-24 (|a| + |b|)^2 / (2 d) + 2^-23 d: the norms and
the dot product are sums of D exact products accumulated in fp32, d^2 = |a|^2 + |b|^2 - 2 a.b carries
(D + 2) 2^-24 (|a| + |b|)^2 at most, d = sqrt(d^2) divides that by 2 d, and the square root and the last sum
round once more. A radius (fp16 of a distance) may therefore differ from the fp16 rounding of the fp64
distance only where that distance lies within the band of an fp16 rounding boundary, and then by one fp16 step.
For the radii D = 32: at D = 256 the fp64 criterion alone excuses about 4 % of the rows (the band grows with
D^1.5, the fp16 spacing with D^0.5), past the 1 % cap; the hits fixture keeps D = 256.

Frechet fixture: a stand-in detector and autoencoder whose outputs are the same bits on every IEEE machine
(exact integer sums scaled by a power of two; elementwise fp32 arithmetic), so the reference's value recorded
in the golden file is reproducible from the images. (A first form with a square root on the features gave
statistics that depend on the host BLAS's summation order; the near-singular covariance of these correlated
features turned that last-bit difference into 2.5e-5 of FID between two hosts.)"""
import os
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_golden.npz")

NHOOD = 3
LATTICE = [(300, 257, 8, 12, 0), (513, 640, 72, 16, 2), (1031, 901, 200, 20, 1)]     # N, M, D, C, seed
GAUSS_RADII = (1536, 32, 0)                                                          # N, D, seed
GAUSS_HITS = (1536, 1536, 256, 0)                                                    # N, P, D, seed
WIDE = (257, 4096, 3)                                                                # N, D, seed (the VGG width)
CHUNKS = [1, 17, 64, 3, 50, 33, 32]                                                  # 7 uneven appends, 200 rows
STATS_D = 24


def tag(case):
    return "x".join(str(v) for v in case)


def lattice(N, M, D, C, seed):
    """(real [N, D], gen [M, D]) fp32 arrays of small integers."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(-6, 7, (C, D))
    q = (3 * C) // 4
    real = centres[rng.integers(0, q, N)]
    gen = centres[C - q + rng.integers(0, q, M)]
    w = min(8, D)
    real[:, :w] += rng.integers(-1, 2, (N, w))
    gen[:, :w] += rng.integers(-1, 2, (M, w))
    return real.astype(np.float32), gen.astype(np.float32)


def gaussian(N, P, D, seed):
    """(manifold [N, D], probes [P, D]) fp16 tensors."""
    g = torch.Generator().manual_seed(seed)
    manifold = torch.randn(N, D, generator=g).to(torch.float16)
    probes = (0.97 * torch.randn(P, D, generator=g) + 0.02).to(torch.float16)
    return manifold, probes


def dist64(a, b):
    """fp64 Euclidean distances [rows of a, rows of b] (the expanded form in fp64: its own error is 2^-29 of the
    fp32 band)."""
    a, b = a.double(), b.double()
    d2 = a.pow(2).sum(1)[:, None] + b.pow(2).sum(1)[None, :] - 2 * (a @ b.T)
    return d2.clamp_min(0).sqrt()


def band(na, nb, d, D):
    """The fp32-against-fp64 error bound of a distance d between rows of norms na, nb (module docstring)."""
    return (D + 2) * 2.0 ** -24 * (na + nb) ** 2 / (2 * d.clamp_min(1e-30)) + 2.0 ** -23 * d


def fp16_neighbours(h):
    """(previous, next) fp16 value of the positive finite fp16 tensor h, as fp64."""
    bits = h.view(torch.int16)
    return (bits - 1).view(torch.float16).double(), (bits + 1).view(torch.float16).double()


def radius_rule(feats, k):
    """fp64 reference of knn_radius on fp16 feats: (expected fp16 radii, excused bool [N]). A row is excused (its
    radius may be one fp16 step off) iff its fp64 (k + 1)-th distance lies within the band of an fp16 rounding
    boundary."""
    D = feats.shape[1]
    d = dist64(feats, feats)
    kth, j = d.kthvalue(k + 1, dim=1)
    norms = feats.double().norm(dim=1)
    bnd = band(norms, norms[j], kth, D)
    h = kth.to(torch.float16)
    lo, hi = fp16_neighbours(h)
    mid_lo, mid_hi = (h.double() + lo) / 2, (h.double() + hi) / 2
    excused = (kth - mid_lo <= bnd) | (mid_hi - kth <= bnd)
    return h, excused


def check_radii(got, feats, k, cap):
    """The rule above on kernel radii `got` (fp16 [N]); returns the excused share. cap: the largest share of
    excused rows allowed (None: no cap)."""
    h, excused = radius_rule(feats, k)
    got = got.cpu()
    assert got.dtype == torch.float16 and got.shape == h.shape
    assert torch.equal(got[~excused], h[~excused])
    lo, hi = fp16_neighbours(h)
    g = got.double()
    assert ((g == h.double()) | (g == lo) | (g == hi))[excused].all()
    share = float(excused.double().mean())
    if cap is not None:
        assert share <= cap, share
    return share


def hits_rule(probes, manifold, radii):
    """fp64 reference of manifold_hits: (expected bool [P], excused bool [P]). A row is excused iff it has no clear
    hit (d <= r - band) and some pair inside the band (|d - r| <= band)."""
    D = probes.shape[1]
    d = dist64(probes, manifold)
    r = radii.double()[None, :]
    bnd = band(probes.double().norm(dim=1)[:, None], manifold.double().norm(dim=1)[None, :], d, D)
    expect = (d <= r).any(dim=1)
    clear = (d <= r - bnd).any(dim=1)
    near = ((d - r).abs() <= bnd).any(dim=1)
    return expect, (~clear) & near


# ------------------------------------------------------------------------------------------ statistics

def stats_fixture(kind):
    """[200, STATS_D] fp32: 'int' small integers (every sum exact in fp64), 'float' randn."""
    rng = np.random.default_rng(7)
    if kind == "int":
        return rng.integers(-8, 9, (sum(CHUNKS), STATS_D)).astype(np.float32)
    return rng.standard_normal((sum(CHUNKS), STATS_D)).astype(np.float32)


def chunks(x, sizes=CHUNKS):
    at = 0
    for n in sizes:
        yield x[at:at + n]
        at += n


def cov_bound(x):
    """Elementwise bound on |raw_cov - exact|: 2 n 2^-53 (|X|^T |X|)_ij (products of widened fp32 values are exact
    in fp64; only the n additions round)."""
    a = np.abs(x.astype(np.float64))
    return 2 * x.shape[0] * 2.0 ** -53 * (a.T @ a)


# ------------------------------------------------------------------------- stand-in detector, autoencoder, data

FID_ITEMS, FID_RES, FID_D = 96, 16, 16


class StandInDetector(torch.nn.Module):
    """features = 2^-8 W . pixels with small non-negative integer W on the 16 x 16 pooled uint8 image: the sums are
    exact integers below 2^20 in fp32 in any order, so the features are the same bits on every machine, and so are
    their fp64 sums and cross products over the 96 items (47 bits at most): the statistics do not depend on the
    batching or on the BLAS kernel that adds them up."""

    def __init__(self, num_features=FID_D, seed=0):
        super().__init__()
        rng = np.random.default_rng(seed)
        w = rng.integers(0, 4, (num_features, 3 * FID_RES * FID_RES)).astype(np.float32)
        self.register_buffer("w", torch.from_numpy(w))

    def forward(self, img, return_features: bool = False):
        x = torch.nn.functional.adaptive_avg_pool2d(img.to(torch.float32), [16, 16]).flatten(1)
        return torch.matmul(x, self.w.t()) * 0.00390625


class StandInG(torch.nn.Module):
    """An 'autoencoder' with the generator's call: G(real in [0, 1], c, validation=True).gen_img in [-1, 1]."""

    def __init__(self):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.tensor(0.875))

    def forward(self, img, c, validation=False):
        x = img * 2 - 1
        return types.SimpleNamespace(gen_img=x * self.gain + 0.0625 * torch.roll(x, 1, dims=-1))


class TinyImageDataset(torch.utils.data.Dataset):
    """Map-style dataset of seeded uint8 images with blocky structure (so the pooled features vary)."""

    def __init__(self, path="tiny", num_items=FID_ITEMS, resolution=FID_RES, seed=0, max_size=None, xflip=False):
        rng = np.random.default_rng(seed)
        base = rng.integers(0, 256, (num_items, 3, 4, 4))
        img = np.repeat(np.repeat(base, resolution // 4, axis=2), resolution // 4, axis=3)
        img = np.clip(img + rng.integers(-20, 21, img.shape), 0, 255)
        self.images = img.astype(np.uint8)

    def __len__(self):
        return self.images.shape[0]

    def __getitem__(self, i):
        return self.images[i], np.zeros([0], dtype=np.float32)


def fid_features():
    """(real, gen) fp32 feature arrays of the stand-ins over the whole TinyImageDataset."""
    ds, det, G = TinyImageDataset(), StandInDetector(), StandInG()
    img = torch.from_numpy(ds.images)
    with torch.no_grad():
        real = det(img)
        out = G(img.to(torch.float32) / 255., None, validation=True).gen_img
        gen = det((out * 127.5 + 128).clamp(0, 255).to(torch.uint8))
    return real.numpy(), gen.numpy()


def write_detectors(folder):
    """TorchScript stand-ins under the file stems the metrics ask for."""
    os.makedirs(folder, exist_ok=True)
    for stem in ("inception-2015-12-05", "vgg16"):
        torch.jit.script(StandInDetector()).save(os.path.join(folder, stem + ".pt"))
    return folder


def golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}
