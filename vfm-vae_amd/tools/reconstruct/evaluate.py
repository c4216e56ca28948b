"""LPIPS / PSNR / SSIM between paired image folders (reconstruction quality).

Drop-in for the reference `tools/reconstruct/evaluate.py:22-139`: same CLI
(`--ref-dir --pred-dir --batch-size --num-workers`), pairs = the sorted intersection of the
two folders' file names, images mapped to [-1, 1], and the same reductions:
  * LPIPS (`training.lpips.LPIPS`): batch mean, weighted by batch size;
  * SSIM: torchmetrics `StructuralSimilarityIndexMeasure(data_range=2)` restated in
    `training.loss.SSIM` (11×11 Gaussian σ=1.5, reflect pad, border cropped), batch mean;
  * PSNR: per image `10·log10(2² / mse)` (torchmetrics `PeakSignalNoiseRatio(data_range=2)`
    called one image at a time, as the reference does), averaged.
torchmetrics is not installed here, so SSIM/PSNR parity rests on the restatement (unpinned).

Beyond the reference's CLI: `--metrics fid pr [--detector-dir DIR] [--nhood-size 3]` adds the Frechet distance
and improved precision / recall between the two folders through the metrics package
(`evaluate_distribution_metrics`); without the flag nothing changes.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import common  # noqa: E402


def psnr_per_image(pred, ref, data_range=2.0):
    mse = (pred.double() - ref.double()).pow(2).flatten(1).mean(1)
    return 10.0 * torch.log10(data_range ** 2 / mse)


@torch.no_grad()
def evaluate_image_metrics(ref_dir, pred_dir, batch_size=64, num_workers=8, device=None, log=print):
    from training.lpips import LPIPS
    from training.loss import SSIM
    device = torch.device(device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    log(f"Using device: {device}")
    names = sorted(set(os.listdir(ref_dir)) & set(os.listdir(pred_dir)))
    if not names:
        raise ValueError(f"No overlapping files found between {ref_dir} and {pred_dir}")
    lpips_metric = LPIPS().to(device).eval()
    ssim_metric = SSIM(data_range=2.0)
    pool = common.Writer(workers=max(1, num_workers)).pool

    def load(batch):
        ref = [common.load_png_uint8(os.path.join(ref_dir, n)) for n in batch]
        prd = [common.load_png_uint8(os.path.join(pred_dir, n)) for n in batch]
        return ref, prd

    batches = [names[i:i + batch_size] for i in range(0, len(names), batch_size)]
    lp_sum = ps_sum = ss_sum = 0.0
    total = 0
    fut = pool.submit(load, batches[0])
    for bi in range(len(batches)):
        ref_a, prd_a = fut.result()
        if bi + 1 < len(batches):
            fut = pool.submit(load, batches[bi + 1])
        ref = common.batch_to_device(ref_a, device).sub_(0.5).div_(0.5)
        prd = common.batch_to_device(prd_a, device).sub_(0.5).div_(0.5)
        bs = ref.shape[0]
        lp = lpips_metric(prd, ref).mean()
        ss = ssim_metric(prd, ref)
        pn = psnr_per_image(prd, ref).mean()
        lp_sum += float(lp) * bs
        ss_sum += float(ss) * bs
        ps_sum += float(pn) * bs
        total += bs
    pool.shutdown(wait=True)
    res = {"total": total, "lpips": lp_sum / total, "psnr": ps_sum / total, "ssim": ss_sum / total}
    log("\n===== Evaluation Results =====")
    log(f"Total Images : {total}")
    log(f"Average LPIPS: {res['lpips']:.4f}")
    log(f"Average PSNR : {res['psnr']:.4f}")
    log(f"Average SSIM : {res['ssim']:.4f}")
    return res


@torch.no_grad()
def evaluate_distribution_metrics(ref_dir, pred_dir, metrics=("fid", "pr"), detector_dir=None, nhood_size=3,
                                  batch_size=64, num_workers=8, device=None, log=print):
    """FID and improved precision / recall between the images of --ref-dir (the real set) and of --pred-dir (the
    reconstructions), through the metrics package: detector features of both folders into FeatureStats (on the
    fidstats kernel on a GPU), frechet_distance, and knn_radius / manifold_hits. The detectors (Inception-v3 for
    fid, VGG16 for pr) are files in --detector-dir (else VFM_DETECTOR_DIR, else the dnnlib cache)."""
    from metrics import frechet_inception_distance as fid_mod, metric_utils, precision_recall
    unknown = sorted(set(metrics) - {"fid", "pr"})
    if unknown:
        raise ValueError(f"unknown metrics {unknown}; choose from fid, pr")
    if detector_dir is not None:
        os.environ["VFM_DETECTOR_DIR"] = str(detector_dir)
    device = torch.device(device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    names = sorted(set(os.listdir(ref_dir)) & set(os.listdir(pred_dir)))
    if not names:
        raise ValueError(f"No overlapping files found between {ref_dir} and {pred_dir}")
    pool = common.Writer(workers=max(1, num_workers)).pool
    batches = [names[i:i + batch_size] for i in range(0, len(names), batch_size)]
    res = {"total": len(names)}
    for metric in metrics:
        url = fid_mod.INCEPTION_URL if metric == "fid" else precision_recall.VGG16_URL
        detector = metric_utils.get_feature_detector(url, device=device)
        kw = dict(capture_mean_cov=True) if metric == "fid" else dict(capture_all=True)
        stats = {}
        for side, folder in (("ref", ref_dir), ("pred", pred_dir)):
            stats[side] = metric_utils.FeatureStats(**kw)
            load = lambda batch, folder=folder: [common.load_png_uint8(os.path.join(folder, n)) for n in batch]
            fut = pool.submit(load, batches[0])
            for bi in range(len(batches)):
                arrays = fut.result()
                if bi + 1 < len(batches):
                    fut = pool.submit(load, batches[bi + 1])
                images = torch.from_numpy(np.stack(arrays)).to(device).permute(0, 3, 1, 2).contiguous()   # uint8 RGB
                stats[side].append_torch(detector(images, return_features=True))
        if metric == "fid":
            mu_r, sigma_r = stats["ref"].get_mean_cov()
            mu_p, sigma_p = stats["pred"].get_mean_cov()
            res["fid"] = fid_mod.frechet_distance(mu_p, sigma_p, mu_r, sigma_r)
        else:
            real = stats["ref"].get_all_torch().to(torch.float16).to(device)
            gen = stats["pred"].get_all_torch().to(torch.float16).to(device)
            res["precision"] = precision_recall.manifold_fraction(real, gen, nhood_size)
            res["recall"] = precision_recall.manifold_fraction(gen, real, nhood_size)
    pool.shutdown(wait=True)
    if "fid" in res:
        log(f"FID          : {res['fid']:.4f}")
    if "precision" in res:
        log(f"Precision    : {res['precision']:.4f}")
        log(f"Recall       : {res['recall']:.4f}")
    return res


if __name__ == "__main__":
    import argparse
    p = argparse.ArgumentParser(description="Evaluate LPIPS / PSNR / SSIM between image pairs.")
    p.add_argument("--ref-dir", type=str, required=True, help="Path to reference images.")
    p.add_argument("--pred-dir", type=str, required=True, help="Path to predicted images.")
    p.add_argument("--batch-size", type=int, default=64, help="Batch size for GPU inference.")
    p.add_argument("--num-workers", type=int, default=8, help="Number of loader threads.")
    p.add_argument("--metrics", nargs="+", choices=["fid", "pr"], default=None,
                   help="Also compute FID and / or precision / recall between the two folders.")
    p.add_argument("--detector-dir", type=str, default=None, help="Folder with the detector files (fid, pr).")
    p.add_argument("--nhood-size", type=int, default=3, help="Neighbourhood size of precision / recall.")
    a = p.parse_args()
    evaluate_image_metrics(a.ref_dir, a.pred_dir, batch_size=a.batch_size, num_workers=a.num_workers)
    if a.metrics:
        evaluate_distribution_metrics(a.ref_dir, a.pred_dir, metrics=a.metrics, detector_dir=a.detector_dir,
                                      nhood_size=a.nhood_size, batch_size=a.batch_size, num_workers=a.num_workers)
