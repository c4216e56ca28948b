"""Frechet distance between the Inception feature statistics of the dataset and of its reconstructions (rFID;
reference metrics/frechet_inception_distance.py). The statistics are accumulated on the device
(metric_utils.FeatureStats on torch_utils.ops.fidstats_hip); the distance itself -- one matrix square root of a
D x D product per metric -- is not a hot path and stays scipy fp64 on the host of rank 0, as in the reference."""
import numpy as np
import scipy.linalg

from . import metric_utils

INCEPTION_URL = ('https://api.ngc.nvidia.com/v2/models/nvidia/research/stylegan3/versions/1/files/metrics/'
                 'inception-2015-12-05.pkl')


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr(sigma1 + sigma2 - 2 sqrtm(sigma1 sigma2)), fp64 (generated statistics first, as the
    reference orders the product)."""
    m = np.square(mu1 - mu2).sum()
    s, _ = scipy.linalg.sqrtm(np.dot(sigma1, sigma2), disp=False)
    return float(np.real(m + np.trace(sigma1 + sigma2 - s * 2)))


def compute_fid(opts, max_real, num_gen):
    detector_kwargs = dict(return_features=True)       # the raw pool features, before the classifier
    mu_real, sigma_real = metric_utils.compute_feature_stats_for_dataset(
        opts=opts, detector_url=INCEPTION_URL, detector_kwargs=detector_kwargs, rel_lo=0, rel_hi=0,
        capture_mean_cov=True, max_items=max_real).get_mean_cov()
    mu_gen, sigma_gen = metric_utils.compute_feature_stats_for_generator(
        opts=opts, detector_url=INCEPTION_URL, detector_kwargs=detector_kwargs, rel_lo=0, rel_hi=1,
        capture_mean_cov=True, max_items=num_gen).get_mean_cov()
    if opts.rank != 0:
        return float('nan')
    return frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real)
