"""Frechet Inception Distance (reference: metrics/frechet_inception_distance.py:19-71).

    mu, sigma = mean / covariance (np.cov, rowvar=False) of the feature activations of `num_images` reals and fakes
    FID = |mu_f - mu_r|^2 + trace(sigma_f + sigma_r - 2 sqrtm(sigma_f sigma_r)),   real part            (:64-71)

The Inception-v3 feature network of the reference (metrics/inception_v3_features.pkl) is not available; the metric takes
`feature_fn(uint8 images [n, C, H, W] on the device) -> [n, F] array / tensor` instead.

Features that come back as device tensors stay on the device: every minibatch is folded into a `hip_ops.FeatureMoments`
(csrc/moments.hip: fp64 sums and second moments on the f64 matrix instruction, shifted by the first minibatch's column mean)
and (mu, sigma) is the one device -> host copy of a feature set.  Features that come back as NumPy arrays or CPU tensors are
collected on the host and go through np.mean / np.cov, the reference's statements.  Real statistics are kept per object and,
for a TFRecord data set and a named `feature_fn`, in the reference's .stylegan2-cache file (:32-45).

Under a process group (`run(..., process_group=)`, one process per GPU) the images are dealt to the ranks the way the
reference's per-GPU towers spread them (:49-57; `MetricBase._walk` states the dealing).  Every rank folds its rows into its
own FeatureMoments, `FeatureMoments.all_merge` leaves every rank with the bit-identical union (csrc/moments.hip:
igan_moments_merge), every rank finalises and checks mu, and rank 0 alone evaluates the distance and reports.  The cache file
is read and written by rank 0 only (what it writes is the merged statistics).  Host features are REFUSED under a group: they
are evaluated by one process."""
import os

import numpy as np
import scipy.linalg
import torch

from .. import hip_ops
from . import metric_base
from .metric_base import SHARD_SEED, shard_slices  # noqa: F401  (the dealing lives in metric_base; both names stay importable here)


def fid_from_statistics(mu_real, sigma_real, mu_fake, sigma_fake):
    m = np.square(mu_fake - mu_real).sum()
    s, _ = scipy.linalg.sqrtm(np.dot(sigma_fake, sigma_real), disp=False)
    dist = m + np.trace(sigma_fake + sigma_real - 2 * s)
    return np.real(dist)


def statistics(activations):
    return np.mean(activations, axis=0), np.cov(activations, rowvar=False)


def fid_from_activations(act_real, act_fake):
    return fid_from_statistics(*statistics(act_real), *statistics(act_fake))


class _Activations:
    """The feature rows of one set as they arrive: device tensors feed a hip_ops.FeatureMoments, anything else the host array
    of the reference; `statistics(what)` -> (mu, sigma) of either."""

    def __init__(self, metric):
        self.metric, self.moments, self.host, self.count = metric, None, None, 0

    def add(self, f):
        on_device = torch.is_tensor(f) and f.is_cuda
        self.metric._same_kind(self.count == 0, on_device, self.moments is not None, 'feature_fn')
        if on_device:
            if self.moments is None:
                self.moments = hip_ops.FeatureMoments(f.shape[1], f.device)
            self.moments.update(f)
        else:
            f = f.detach().numpy() if torch.is_tensor(f) else np.asarray(f)
            if self.host is None:
                self.host = np.empty([self.metric.num_images, f.shape[1]], dtype=np.float32)
            self.host[self.count:self.count + f.shape[0]] = f
        self.count += f.shape[0]

    def statistics(self, what):
        return _finite_mu(*(self.moments.finalize() if self.moments is not None else statistics(self.host)), what)


def _finite_mu(mu, sigma, what):
    """(mu, sigma) as given, unless a column of mu is NaN or infinite: then no distance can be computed."""
    bad = int(np.count_nonzero(~np.isfinite(mu)))
    if bad:
        raise FloatingPointError('FID: %d of the %d columns of mu of the %s features are non-finite: feature_fn returned NaN or '
                                 'infinity; no distance is computed' % (bad, mu.shape[0], what))
    return mu, sigma


class FID(metric_base.MetricBase):
    multi_rank = True

    def __init__(self, num_images, minibatch_per_gpu, feature_fn=None, **kwargs):
        super().__init__(**kwargs)
        self.num_images = num_images
        self.minibatch_per_gpu = minibatch_per_gpu
        self.feature_fn = feature_fn
        self._real_stats = None

    def _statistics(self, batches, what):
        """(mu, sigma) of the feature rows of `batches`, one [n, F] array / tensor per minibatch."""
        acc = _Activations(self)
        for f in batches:
            acc.add(f)
        return acc.statistics(what)

    def _walk_statistics(self, Gs, Gs_kwargs, which, num_gpus):
        """One process: (mu, sigma) of the features of the 'real' or 'fake' images, folded minibatch by minibatch."""
        acc = _Activations(self)
        self._walk(Gs, Gs_kwargs, which, self.feature_fn, lambda begin, end, f: acc.add(f), 'result', num_gpus=num_gpus)
        return acc.statistics(which)

    # ---- under a process group: every rank folds its rows, the states are merged on the device --------------------------------
    def _shard_moments(self, Gs, Gs_kwargs, which, rank, world):
        """hip_ops.FeatureMoments of the 'real' or 'fake' rows that rank `rank` of `world` owns (MetricBase._walk), or None when
        it owns none.  A function of its arguments and the data set alone, so one process can rebuild every rank's state."""
        acc = _Activations(self)
        self._walk(Gs, Gs_kwargs, which, self.feature_fn, lambda begin, end, f: acc.add(self._device_result(f, 'feature_fn')), 'result',
                   shard=(rank, world))
        return acc.moments

    def _merged_statistics(self, moments, device, what):
        """(mu, sigma) of the union of all ranks' rows, the same bits on every rank; every rank checks mu, so a non-finite
        feature on one rank raises on all of them and nobody is left at a collective."""
        F = self._agree_on_width(moments.F if moments is not None else 0, device, what + ' feature')
        if moments is None:
            moments = hip_ops.FeatureMoments(F, device, chunk_rows=1)
        moments.all_merge(self._process_group)
        return _finite_mu(*moments.finalize(), what)

    def _evaluate_sharded(self, Gs, Gs_kwargs):
        from ..training import misc
        dist, group = torch.distributed, self._process_group
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        root = dist.get_global_rank(group, 0)
        cache_file = self._get_cache_file_for_reals(feature_fn=self.feature_fn, num_images=self.num_images)
        # rank 0 decides whether the reals are evaluated (its object's statistics, else the file): one decision for all ranks
        need = torch.zeros(1, device=Gs.device, dtype=torch.int64)
        if rank == 0 and self._real_stats is None:
            if cache_file is not None and os.path.isfile(cache_file):
                self._real_stats = tuple(misc.load_pkl(cache_file))
            else:
                need += 1
        dist.broadcast(need, root, group=group)
        if int(need.item()):
            self._real_stats = self._merged_statistics(self._shard_moments(Gs, Gs_kwargs, 'real', rank, world), Gs.device, 'real')
            if rank == 0 and cache_file is not None:        # the merged statistics, written once
                os.makedirs(os.path.dirname(cache_file), exist_ok=True)
                misc.save_pkl(self._real_stats, cache_file)
        mu_fake, sigma_fake = self._merged_statistics(self._shard_moments(Gs, Gs_kwargs, 'fake', rank, world), Gs.device, 'fake')
        if rank == 0:
            mu_real, sigma_real = self._real_stats
            self._report_result(fid_from_statistics(mu_real, sigma_real, mu_fake, sigma_fake))

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        from ..training import misc
        if self.feature_fn is None:
            raise RuntimeError('FID needs feature_fn: the reference\'s metrics/inception_v3_features.pkl is not available in this tree')
        if self._process_group is not None:
            return self._evaluate_sharded(Gs, Gs_kwargs)
        if self._real_stats is None:
            cache_file = self._get_cache_file_for_reals(feature_fn=self.feature_fn, num_images=self.num_images)
            if cache_file is not None and os.path.isfile(cache_file):
                self._real_stats = tuple(misc.load_pkl(cache_file))
            else:
                self._real_stats = self._walk_statistics(Gs, Gs_kwargs, 'real', num_gpus)
                if cache_file is not None:
                    os.makedirs(os.path.dirname(cache_file), exist_ok=True)
                    misc.save_pkl(self._real_stats, cache_file)
        mu_real, sigma_real = self._real_stats
        mu_fake, sigma_fake = self._walk_statistics(Gs, Gs_kwargs, 'fake', num_gpus)
        self._report_result(fid_from_statistics(mu_real, sigma_real, mu_fake, sigma_fake))
