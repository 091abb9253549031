"""Frechet Inception Distance (reference: metrics/frechet_inception_distance.py:19-71).

    mu, sigma = mean / covariance (np.cov, rowvar=False) of the feature activations of `num_images` reals and fakes
    FID = |mu_f - mu_r|^2 + trace(sigma_f + sigma_r - 2 sqrtm(sigma_f sigma_r)),   real part            (:64-71)

The Inception-v3 feature network of the reference (metrics/inception_v3_features.pkl) is not available; the metric takes
`feature_fn(uint8 images [n, C, H, W] on the device) -> [n, F] array / tensor` instead.

Features that come back as device tensors stay on the device: every minibatch is folded into a `hip_ops.FeatureMoments`
(csrc/moments.hip: fp64 sums and second moments on the f64 matrix instruction, shifted by the first minibatch's column mean)
and (mu, sigma) is the one device -> host copy of a feature set.  Features that come back as NumPy arrays or CPU tensors are
collected on the host and go through np.mean / np.cov, the reference's statements.  Real statistics are kept per object and,
for a TFRecord data set and a named `feature_fn`, in the reference's .stylegan2-cache file (:32-45)."""
import os

import numpy as np
import scipy.linalg

from . import metric_base


def fid_from_statistics(mu_real, sigma_real, mu_fake, sigma_fake):
    m = np.square(mu_fake - mu_real).sum()
    s, _ = scipy.linalg.sqrtm(np.dot(sigma_fake, sigma_real), disp=False)
    dist = m + np.trace(sigma_fake + sigma_real - 2 * s)
    return np.real(dist)


def statistics(activations):
    return np.mean(activations, axis=0), np.cov(activations, rowvar=False)


def fid_from_activations(act_real, act_fake):
    return fid_from_statistics(*statistics(act_real), *statistics(act_fake))


class FID(metric_base.MetricBase):
    def __init__(self, num_images, minibatch_per_gpu, feature_fn=None, **kwargs):
        super().__init__(**kwargs)
        self.num_images = num_images
        self.minibatch_per_gpu = minibatch_per_gpu
        self.feature_fn = feature_fn
        self._real_stats = None

    def _statistics(self, batches, what):
        """(mu, sigma) of the feature rows of `batches`: device tensors feed a FeatureMoments, anything else the host array."""
        import torch
        moments = activations = None
        begin = 0
        for f in batches:
            on_device = torch.is_tensor(f) and f.is_cuda
            if begin and on_device != (moments is not None):
                raise RuntimeError('FID: feature_fn must return device tensors for every minibatch or for none')
            if on_device:
                if moments is None:
                    from .. import hip_ops
                    moments = hip_ops.FeatureMoments(f.shape[1], f.device)
                moments.update(f)
            else:
                f = f.detach().numpy() if torch.is_tensor(f) else np.asarray(f)
                if activations is None:
                    activations = np.empty([self.num_images, f.shape[1]], dtype=np.float32)
                activations[begin:begin + f.shape[0]] = f
            begin += f.shape[0]
        mu, sigma = moments.finalize() if moments is not None else statistics(activations)
        bad = int(np.count_nonzero(~np.isfinite(mu)))
        if bad:
            raise FloatingPointError('FID: %d of the %d columns of mu of the %s features are non-finite: feature_fn returned NaN or '
                                     'infinity; no distance is computed' % (bad, mu.shape[0], what))
        return mu, sigma

    def _real_features(self, minibatch_size, device):
        import torch
        for idx, images in enumerate(self._iterate_reals(minibatch_size=minibatch_size)):
            begin = idx * minibatch_size
            end = min(begin + minibatch_size, self.num_images)
            yield self.feature_fn(torch.from_numpy(images[:end - begin]).to(device))
            if end == self.num_images:
                break

    def _fake_features(self, Gs, minibatch_size, Gs_kwargs):
        for begin in range(0, self.num_images, minibatch_size):
            end = min(begin + minibatch_size, self.num_images)
            yield self.feature_fn(self._generate(Gs, minibatch_size, Gs_kwargs))[:end - begin]

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        from ..training import misc
        if self.feature_fn is None:
            raise RuntimeError('FID needs feature_fn: the reference\'s metrics/inception_v3_features.pkl is not available in this tree')
        minibatch_size = num_gpus * self.minibatch_per_gpu
        if self._real_stats is None:
            cache_file = self._get_cache_file_for_reals(feature_fn=self.feature_fn, num_images=self.num_images)
            if cache_file is not None and os.path.isfile(cache_file):
                self._real_stats = tuple(misc.load_pkl(cache_file))
            else:
                self._real_stats = self._statistics(self._real_features(minibatch_size, Gs.device), 'real')
                if cache_file is not None:
                    os.makedirs(os.path.dirname(cache_file), exist_ok=True)
                    misc.save_pkl(self._real_stats, cache_file)
        mu_real, sigma_real = self._real_stats
        mu_fake, sigma_fake = self._statistics(self._fake_features(Gs, minibatch_size, Gs_kwargs), 'fake')
        self._report_result(fid_from_statistics(mu_real, sigma_real, mu_fake, sigma_fake))
