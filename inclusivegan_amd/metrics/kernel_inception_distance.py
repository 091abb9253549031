"""Kernel Inception Distance (Binkowski et al., "Demystifying MMD GANs", ICLR 2018; the `kid50k` of later StyleGAN code bases).
The reference has no such metric: like dc50k5 this one is the project's own.

    k(a, b)    = (a.b / F + 1)^3                                  cubic polynomial kernel on F-dimensional features
    subset s   : m = min(num_real, num_fake, max_subset_size) fakes x_i and m reals y_j, drawn without replacement
    t_s        = (sum_{i != j} k(x_i, x_j) + sum_{i != j} k(y_i, y_j)) / (m - 1) - 2 sum_{i, j} k(x_i, y_j) / m
    kid        = (t_0 + t_1 + ... + t_{S-1}) / S / m              subsets added in order, fp64

the published code's `a.sum() - diag(a).sum()` with a = Kxx + Kyy and `b.sum()` with b = Kxy.  It is the UNBIASED estimator of
MMD^2, which is why it is the number to use where FID is not: FID's bias grows as the sample shrinks, so two FIDs taken at
different N -- a minority subgroup of a few hundred reals against the full set -- are not comparable; two KIDs are.

The draw order is part of the contract (`kid_subsets`): ONE `np.random.RandomState(seed)`; for every subset in order first
`choice(num_fake, m, replace=False)`, then `choice(num_real, m, replace=False)`.

The three sums of every subset come from ONE launch of `igan_poly3_kernel_sums` (csrc/poly_kernel_sum.hip): rows gathered by
index, features widened to fp64, dot products on the f64 matrix instruction, the cube in fp64, every addition in a fixed order
without atomics.  The result is a difference of O(1) means that is itself 1e-3 ... 1e-5, and fp32 sums move each mean by
1e-8 ... 1e-7 of itself: two to three digits of a small kid are left (profiles/kid.txt).  Row s of `sums` depends on subset s alone, so under `process_group=` rank r evaluates the subsets s with
s mod world == r, the rows are gathered and put back in subset order -- moved, never summed -- and every rank holds the
one-process `sums` bit for bit and computes `kid` itself.  `real_rows=` restricts the reals to a subgroup (for example
`np.nonzero(labels[:, a])[0]`) by mapping the drawn positions through it: the feature matrix is not copied.

`KID` takes `feature_fn(uint8 images [n, C, H, W] on the device) -> [n, F] array / tensor`, like `DC`."""
import numpy as np
import torch

from .. import dnnlib
from .. import hip_ops
from . import metric_base
from .precision_recall import _to_device


def kid_subsets(num_real, num_fake, num_subsets, max_subset_size, seed):
    """The subsets of a KID evaluation -> (idx_fake int64 [S, m], idx_real int64 [S, m], m), m = min(num_real, num_fake,
    max_subset_size).  Host only.  One RandomState(seed); per subset, in order: choice(num_fake, m, replace=False), then
    choice(num_real, m, replace=False)."""
    num_real, num_fake, num_subsets, max_subset_size = int(num_real), int(num_fake), int(num_subsets), int(max_subset_size)
    if num_subsets < 1:
        raise ValueError('kid_subsets: num_subsets must be at least 1')
    m = min(num_real, num_fake, max_subset_size)
    if m < 2:
        raise ValueError('kid_subsets: subsets of %d rows (%d reals, %d fakes, max_subset_size %d): the estimator divides by m - 1'
                         % (m, num_real, num_fake, max_subset_size))
    rnd = np.random.RandomState(seed)
    idx_fake = np.empty((num_subsets, m), np.int64)
    idx_real = np.empty((num_subsets, m), np.int64)
    for s in range(num_subsets):
        idx_fake[s] = rnd.choice(num_fake, m, replace=False)
        idx_real[s] = rnd.choice(num_real, m, replace=False)
    return idx_fake, idx_real, m


def kid_from_sums(sums, m):
    """(kid, per_subset [S]) from sums [S, 3] = (sum_{i != j} k(x, x), sum_{i != j} k(y, y), sum_{i, j} k(x, y)) of subsets of m
    rows: t_s = (sxx + syy) / (m - 1) - 2 sxy / m, kid = (t_0 + t_1 + ... in subset order) / S / m, all fp64."""
    sums = np.asarray(sums, np.float64)
    m = int(m)
    if sums.ndim != 2 or sums.shape[1] != 3 or sums.shape[0] < 1 or m < 2:
        raise ValueError('kid_from_sums: sums must be [S, 3] with S >= 1 and m >= 2')
    bad = np.nonzero(~np.isfinite(sums).all(axis=1))[0]
    if bad.size:
        raise FloatingPointError('KID: the kernel sums of subset %d (and %d more of %d) are non-finite: feature_fn returned NaN or '
                                 'infinity, or features too large for the cube' % (int(bad[0]), bad.size - 1, sums.shape[0]))
    per_subset = (sums[:, 0] + sums[:, 1]) / np.float64(m - 1) - 2.0 * sums[:, 2] / np.float64(m)
    total = np.float64(0.0)
    for t in per_subset:
        total = total + t
    return float(total / np.float64(sums.shape[0]) / np.float64(m)), per_subset


def rank_subsets(num_subsets, rank, world):
    """The subsets that rank `rank` of `world` evaluates: s with s mod world == rank, ascending (none when rank >= num_subsets)."""
    num_subsets, rank, world = int(num_subsets), int(rank), int(world)
    if num_subsets < 0 or world < 1 or not 0 <= rank < world:
        raise ValueError('rank_subsets: need num_subsets >= 0 and 0 <= rank < world')
    return np.arange(rank, num_subsets, world)


def kid_sums_rows(real, fake, idx_fake, idx_real, subsets):
    """Rows `subsets` (a list of subset numbers) of the [S, 3] sums -> float64 [len(subsets), 3] on the device, exactly those
    rows of the whole evaluation.  An empty list launches nothing."""
    subsets = np.asarray(subsets, np.int64)
    if subsets.size == 0:
        return torch.empty((0, 3), device=real.device, dtype=torch.float64)
    return hip_ops.poly3_kernel_sums(fake, real, idx_fake[subsets], idx_real[subsets], 1.0 / real.shape[1], 1.0)


def kid_from_features(real_features, fake_features, num_subsets=100, max_subset_size=1000, seed=0, real_rows=None, process_group=None):
    """KID of two sets of feature vectors; NumPy arrays or device tensors [n, F].  -> EasyDict with `kid`, `per_subset` [S],
    `sums` float64 [S, 3] (host; x = fakes, y = reals) and `m`.  `real_rows`: optional host index array that restricts the reals
    to a subgroup; subsets are drawn from len(real_rows) and mapped through it.  `process_group`: every rank of it makes this
    call with the same matrices, draws the same subsets itself and evaluates those with s mod world == rank."""
    real, fake = _to_device(real_features), _to_device(fake_features)
    if fake.shape[1] != real.shape[1]:
        raise ValueError('kid_from_features: feature dimension %d of the fakes does not match the reals\' %d' % (fake.shape[1], real.shape[1]))
    num_real = real.shape[0]
    if real_rows is not None:
        real_rows = np.asarray(real_rows)
        if real_rows.ndim != 1 or not np.issubdtype(real_rows.dtype, np.integer):
            raise ValueError('kid_from_features: real_rows must be a 1-D integer array of row numbers (np.nonzero(mask)[0])')
        if real_rows.size and (int(real_rows.min()) < 0 or int(real_rows.max()) >= real.shape[0]):
            raise ValueError('kid_from_features: real_rows holds row numbers outside [0, %d)' % real.shape[0])
        num_real = int(real_rows.size)
    idx_fake, idx_real, m = kid_subsets(num_real, fake.shape[0], num_subsets, max_subset_size, seed)
    if real_rows is not None:
        idx_real = real_rows.astype(np.int64)[idx_real]
    S = idx_fake.shape[0]
    if process_group is None:
        sums = kid_sums_rows(real, fake, idx_fake, idx_real, np.arange(S))
    else:
        dist = torch.distributed
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
        own = kid_sums_rows(real, fake, idx_fake, idx_real, rank_subsets(S, rank, world))
        out = torch.empty((S, 3), device=real.device, dtype=torch.float64)
        sums = metric_base.gather_rows(out, [[(int(s), int(s) + 1) for s in rank_subsets(S, r, world)] for r in range(world)], own, process_group)
    state = dnnlib.EasyDict(m=m)
    state.sums = sums.cpu().numpy()
    state.kid, state.per_subset = kid_from_sums(state.sums, m)
    return state


class KID(metric_base.MetricBase):
    """Under a process group the features of both sets are collected by all ranks (MetricBase._feature_matrix: every rank ends
    with the same [num_images, F] matrices) and the subsets are spread over them."""

    multi_rank = True

    def __init__(self, num_images, num_subsets, max_subset_size, minibatch_per_gpu, seed=0, feature_fn=None, **kwargs):
        super().__init__(**kwargs)
        self.num_images = num_images
        self.num_subsets = num_subsets
        self.max_subset_size = max_subset_size
        self.minibatch_per_gpu = minibatch_per_gpu
        self.seed = seed
        self.feature_fn = feature_fn
        self._real_features = None

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        if self.feature_fn is None:
            raise RuntimeError('KID needs feature_fn: no feature network ships with this tree')
        if self._real_features is None:      # cached per object
            self._real_features = self._feature_matrix(Gs, Gs_kwargs, 'real', num_gpus)
        fake_features = self._feature_matrix(Gs, Gs_kwargs, 'fake', num_gpus)
        state = kid_from_features(self._real_features, fake_features, num_subsets=self.num_subsets, max_subset_size=self.max_subset_size,
                                  seed=self.seed, process_group=self._process_group)
        self._report_result(state.kid, fmt='%-10.6f')
