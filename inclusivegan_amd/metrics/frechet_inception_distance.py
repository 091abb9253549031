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

Under a process group (`run(..., process_group=)`, one process per GPU) the work is spread the way the reference's per-GPU
towers spread it (:49-57): a global minibatch is world x minibatch_per_gpu images and rank r owns rows [r mb, (r + 1) mb) of
it (`shard_slices`).  Every rank folds its rows into its own FeatureMoments, `FeatureMoments.all_merge` leaves every rank with
the bit-identical union (csrc/moments.hip: igan_moments_merge), every rank finalises and checks mu, and rank 0 alone evaluates
the distance and reports.  Every rank reads the whole global minibatch of reals from its own data set object and keeps its
rows: the host read is redundant per rank, the real set is exactly the single-process one.  Latents and noise come from a
private device generator seeded per rank, so no two ranks draw the same fakes and the process's device stream is left alone.
The cache file is read and written by rank 0 only (what it writes is the merged statistics).  Host features are REFUSED under a
group: they are evaluated by one process."""
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


def shard_slices(num_images, minibatch_per_gpu, rank, world):
    """The image rows rank `rank` of `world` owns, one (begin, end) per global minibatch: global minibatch g covers images
    [g world mb, (g + 1) world mb) cut at num_images, and the rank owns rows [rank mb, (rank + 1) mb) of it, cut the same way
    (begin == end: the rank sits this minibatch out).  Over the ranks the slices are disjoint and cover [0, num_images)."""
    num_images, mb, rank, world = int(num_images), int(minibatch_per_gpu), int(rank), int(world)
    if mb < 1 or world < 1 or not 0 <= rank < world or num_images < 0:
        raise ValueError('shard_slices: need minibatch_per_gpu >= 1, 0 <= rank < world and num_images >= 0')
    out = []
    for start in range(0, num_images, world * mb):
        begin = min(start + rank * mb, num_images)
        out.append((begin, min(begin + mb, num_images)))
    return out


SHARD_SEED = 0x51d0     # latents and noise of rank r under a process group: a private device generator seeded SHARD_SEED + r


class FID(metric_base.MetricBase):
    multi_rank = True

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

    # ---- under a process group: every rank folds its rows, the states are merged on the device --------------------------------
    def _shard_moments(self, Gs, Gs_kwargs, which, rank, world):
        """hip_ops.FeatureMoments of the 'real' or 'fake' rows that rank `rank` of `world` owns (shard_slices), or None when it
        owns none.  A function of its arguments and the data set alone -- the walk over the reals restarts at image 0, the label
        stream at its seed, latents and noise come from a private device generator seeded SHARD_SEED + rank -- so one process
        can rebuild every rank's state."""
        import torch
        from .. import hip_ops
        from ..dnnlib.tflib import tfutil
        mb = self.minibatch_per_gpu
        slices = shard_slices(self.num_images, mb, rank, world)
        state = []

        def fold(f):
            if not (torch.is_tensor(f) and f.is_cuda):
                raise RuntimeError('FID under a process group: feature_fn must return device tensors; host (NumPy / CPU) features are '
                                   'evaluated by one process only (run without process_group)')
            if not state:
                state.append(hip_ops.FeatureMoments(f.shape[1], f.device))
            state[0].update(f)

        if which == 'real':
            if self._dataset_obj is not None:       # a fresh walk: the real set is the first num_images of the stream
                self._dataset_obj.close()
                self._dataset_obj = None
            # every rank reads the whole global minibatch (the host read is redundant per rank) and keeps its rows
            for g, ((begin, end), images) in enumerate(zip(slices, self._iterate_reals(minibatch_size=world * mb))):
                if end > begin:
                    first = g * world * mb
                    fold(self.feature_fn(torch.from_numpy(images[begin - first:end - first]).to(Gs.device)))
        elif which == 'fake':
            self._label_rng = None
            with tfutil.use_random(tfutil.SeededRandom(Gs.device, SHARD_SEED + rank)):
                for begin, end in slices:
                    labels = self._get_random_labels(world * mb, Gs)[rank * mb:(rank + 1) * mb]      # drawn for the global minibatch
                    if end > begin:
                        fold(self.feature_fn(self._generate(Gs, mb, Gs_kwargs, labels=labels))[:end - begin])
        else:
            raise ValueError('FID._shard_moments: which must be "real" or "fake"')
        return state[0] if state else None

    def _merged_statistics(self, moments, device, what):
        """(mu, sigma) of the union of all ranks' rows, the same bits on every rank; every rank checks mu, so a non-finite
        feature on one rank raises on all of them and nobody is left at a collective."""
        import torch
        from .. import hip_ops
        group = self._process_group
        width = torch.tensor([moments.F if moments is not None else 0], device=device, dtype=torch.int64)
        torch.distributed.all_reduce(width, op=torch.distributed.ReduceOp.MAX, group=group)      # a rank without rows learns F here
        F = int(width.item())
        if F == 0:
            raise ValueError('FID: no rank holds a %s feature row' % what)
        if moments is None:
            moments = hip_ops.FeatureMoments(F, device, chunk_rows=1)
        moments.all_merge(group)
        mu, sigma = moments.finalize()
        bad = int(np.count_nonzero(~np.isfinite(mu)))
        if bad:
            raise FloatingPointError('FID: %d of the %d columns of mu of the %s features are non-finite: feature_fn returned NaN or '
                                     'infinity; no distance is computed' % (bad, mu.shape[0], what))
        return mu, sigma

    def _evaluate_sharded(self, Gs, Gs_kwargs):
        import torch
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
