"""Extract VFM-VAE latent features of an image set for the alignment analysis.

Drop-in for the reference `tools/evaluate_alignment/vaes/extract_features_by_vfm_vae.py`: same CLI
(`--input-dir --output-dir --output-prefix --mode --vae-pth --use-config --resolution --batch-size-per-gpu
--seed`; plus `--device` as on the other tools here), same four modes and folder conventions, same `.pt`
payload:

  clean          <input>/clean/*.png                     -> <prefix>_clean.pt
  noise          <input>/noise_<x.y>/*.png, every level  -> <prefix>_noise_<x.yyy>.pt
  mask           <input>/mask_<x.y>/*.png, every ratio   -> <prefix>_mask_<x.yy>.pt
  equivariance   <input>/clean/<name>.png rotated by record['rotation'] (np.rot90), encoded with
                 eq_scale_factor = record['scale'], is_eq_prior=True, one image at a time, for every name
                 of <input>/equivariance_transforms.json   -> <prefix>_equivariance.pt

  payload {'features': [N, C] fp32, 'names': [...], 'transformations': [...]}, sorted by name;
  features = G.encode(img, eq_scale_factor, is_eq_prior).mean([-2, -1]).

Images are read as the reference's datasets do (RGB, Lanczos resize to resolution x resolution when the size
differs, /255). Launch with torchrun for several GPUs: names are dealt round-robin over ranks and gathered
on rank 0 (the reference's DistributedSampler pads the last round with repeats; the saved set is the same
up to those duplicates). Model overrides, checkpoint loading and process placement are tools/common.py's.
"""
import json
import os
import random
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import common  # noqa: E402

EMPTY_WIDTH = 512           # feature width of the empty tensor the reference saves when nothing was found


def load_rgb(path, resolution, rot=0):
    """HWC float32 in [0, 1]; `rot` degrees counter-clockwise in quarter turns, applied before the scaling."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
        if im.size != (resolution, resolution):
            im = im.resize((resolution, resolution), Image.LANCZOS)
        arr = np.array(im, np.float32)
    if rot:
        arr = np.rot90(arr, k=rot // 90, axes=(0, 1)).copy()
    return arr / 255.0


def list_pngs(folder):
    """(stem, path) of the folder's *.png, sorted by stem."""
    if not os.path.isdir(folder):
        return []
    return sorted((os.path.splitext(f)[0], os.path.join(folder, f)) for f in os.listdir(folder) if f.endswith(".png"))


def scan_levels(base_dir, kind):
    """[(level, folder)] of the `<kind>_<x.y>` sub-folders, ascending level."""
    out = []
    for d in sorted(os.listdir(base_dir)):
        m = re.match(rf"{kind}_(\d+\.\d+)", d)
        if m and os.path.isdir(os.path.join(base_dir, d)):
            out.append((float(m.group(1)), os.path.join(base_dir, d)))
    return sorted(out, key=lambda x: x[0])


def _to_device(arrays, device):
    x = torch.from_numpy(np.stack(arrays)).permute(0, 3, 1, 2)
    if device.type == "cuda":
        x = x.pin_memory().to(device, non_blocking=True)
    return x.contiguous()


@torch.no_grad()
def extract_folder(vae, folder, resolution, batch_size, rank, transformation, log=print):
    """Features of this rank's share of a folder's images, batched."""
    items = rank.shard(list_pngs(folder))
    feats, names = [], []
    for s in range(0, len(items), batch_size):
        batch = items[s:s + batch_size]
        imgs = _to_device([load_rgb(p, resolution) for _, p in batch], rank.device)
        v = vae.encode(imgs, eq_scale_factor=1.0, is_eq_prior=False)
        feats.append(v.mean([-2, -1]).float().cpu())
        names.extend(n for n, _ in batch)
        log(f"[Rank {rank.rank}] {os.path.basename(folder)} {min(s + batch_size, len(items))}/{len(items)}")
    feats = torch.cat(feats, 0) if feats else torch.empty(0, EMPTY_WIDTH)
    return feats, names, [dict(transformation) for _ in names]


@torch.no_grad()
def extract_equivariance(vae, input_dir, resolution, rank, log=print):
    jpath = os.path.join(input_dir, "equivariance_transforms.json")
    if not os.path.exists(jpath):
        if rank.rank == 0:
            log(f"Missing: {jpath}")
        return torch.empty(0, EMPTY_WIDTH), [], []
    with open(jpath, "r") as f:
        records = json.load(f)
    feats, names, trans = [], [], []
    for name in rank.shard(sorted(records.keys())):
        rec = records[name]
        arr = load_rgb(os.path.join(input_dir, "clean", f"{name}.png"), resolution, rot=rec.get("rotation", 0))
        img = _to_device([arr], rank.device)
        v = vae.encode(img, eq_scale_factor=float(rec.get("scale", 1.0)), is_eq_prior=True)   # rotation: done above
        f0 = v[0]
        if f0.ndim > 1:
            f0 = f0.mean([-2, -1])
        feats.append(f0.float().cpu())
        names.append(name)
        trans.append(dict(rec, mode="equivariance"))
    feats = torch.stack(feats, 0) if feats else torch.empty(0, EMPTY_WIDTH)
    return feats, names, trans


def gather_results(f, n, t, rank):
    if rank.world_size > 1:
        gf, gn, gt = ([None] * rank.world_size for _ in range(3))
        torch.distributed.all_gather_object(gf, f)
        torch.distributed.all_gather_object(gn, n)
        torch.distributed.all_gather_object(gt, t)
        if rank.rank != 0:
            return torch.empty(0, EMPTY_WIDTH), [], []
        parts = [x for x in gf if isinstance(x, torch.Tensor) and x.numel() > 0]
        f = torch.cat(parts, 0) if parts else torch.empty(0, EMPTY_WIDTH)
        n = [x for part in gn for x in (part or [])]
        t = [x for part in gt for x in (part or [])]
    return f, n, t


def save_sorted(f, n, t, path, log=print):
    order = sorted(range(len(n)), key=lambda i: n[i])
    f, n, t = f[order], [n[i] for i in order], [t[i] for i in order]
    torch.save({'features': f, 'names': n, 'transformations': t}, path)
    return len(n)


def extract_features(vae, input_dir, output_dir, output_prefix, mode, resolution, batch_size, rank, log=print):
    """Run one mode; returns the files written (rank 0)."""
    if rank.rank == 0:
        os.makedirs(output_dir, exist_ok=True)
    jobs = []                                           # (output file name, folder or None, transformation)
    if mode == 'clean':
        jobs.append((f"{output_prefix}_clean.pt", os.path.join(input_dir, "clean"), {'mode': 'clean'}))
    elif mode == 'equivariance':
        jobs.append((f"{output_prefix}_equivariance.pt", None, None))
    elif mode == 'noise':
        for lvl, d in scan_levels(input_dir, 'noise'):
            jobs.append((f"{output_prefix}_noise_{lvl:.3f}.pt", d, {'mode': 'noise', 'noise_level': lvl}))
    elif mode == 'mask':
        for lvl, d in scan_levels(input_dir, 'mask'):
            jobs.append((f"{output_prefix}_mask_{lvl:.2f}.pt", d, {'mode': 'mask', 'mask_ratio': lvl}))
    else:
        raise ValueError(f"Unknown mode {mode}")
    written = []
    for fname, folder, tf in jobs:
        if folder is None:
            f, n, t = extract_equivariance(vae, input_dir, resolution, rank, log=log)
        else:
            f, n, t = extract_folder(vae, folder, resolution, batch_size, rank, tf, log=log)
        f, n, t = gather_results(f, n, t, rank)
        if rank.rank == 0:
            out = os.path.join(output_dir, fname)
            count = save_sorted(f, n, t, out)
            log(f"Saved {count} {mode} features → {out}")
            written.append(out)
    return written


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="Extract VAE features (pth checkpoint)")
    p.add_argument('--input-dir', type=str, required=True)
    p.add_argument('--output-dir', type=str, required=True)
    p.add_argument('--output-prefix', type=str, required=True)
    p.add_argument('--mode', type=str, choices=['clean', 'noise', 'mask', 'equivariance'], default='clean')
    p.add_argument('--vae-pth', type=str, required=True, help='Path to VAE checkpoint (.pth)')
    p.add_argument('--use-config', type=str, required=True, help='YAML config file')
    p.add_argument('--resolution', type=int, default=256)
    p.add_argument('--batch-size-per-gpu', type=int, default=16)
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--device', type=str, default=None, help='override (default cuda:LOCAL_RANK, else cpu)')
    args = p.parse_args(argv)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)

    rank = common.Rank(args.device)
    if rank.rank == 0:
        print(f"Mode: {args.mode}, Device: {rank.device}, World size: {rank.world_size}")
    vae = common.build_vae(args.use_config, args.resolution, rank.device)
    print(f"Loading checkpoint from: {args.vae_pth}")
    common.load_vae_weights(vae, args.vae_pth, rank.device)
    rank.barrier()
    extract_features(vae, args.input_dir, args.output_dir, args.output_prefix, args.mode, args.resolution,
                     args.batch_size_per_gpu, rank)
    rank.close()


if __name__ == '__main__':
    main()
