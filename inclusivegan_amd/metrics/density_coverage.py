"""Density and coverage (Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative Models", ICML 2020; the
definitions of the `prdc` package).  The reference has no such metric: this one is the project's own.

    radius of a real, neighbourhood k = the value at 0-based position k of its ascending squared distances to ALL reals, itself
                                        included -- `ManifoldEstimator(None, reals, ..., [k]).D[:, 0]`, prdc's
                                        get_kth_value(..., k + 1)
    count[i]                          = #{ j : d2(real_i, fake_j) < radius[i] }
    density                           = sum_i count[i] / (k * M)        (M fakes; int64 sum, one fp64 division)
    coverage                          = #{ i : count[i] > 0 } / N       (N reals)

The radii belong to the REALS only, which is what makes the pair robust where pr50k3's recall is not: one stray fake with a
huge k-NN ball cannot "cover" a region of reals.  The comparison is STRICT (`<`, as in prdc), where pr50k3's membership test is
`<=` (metrics/precision_recall.py): a fake exactly ON a real's sphere is outside here and inside there, and a duplicated real,
whose radius at k = 1 is 0, is covered by nothing, not even by a fake that copies it.  `ball_counts_rows(..., inclusive=True)`
counts with `<=`.

The search is the exact streaming one of pr50k3 (csrc/exact_search.hip): the fp32 MFMA product only screens, a pair it cannot
decide is measured as a direct difference in fp64, so the counts equal an fp64 brute force on the same fp32 features.  The
radii are `precision_recall.ManifoldEstimator`'s, reused; the count is `igan_ball_count_update`, an integer fold with no early
exit, no atomic and no floating-point sum, so rows [b, e) of the pass are exactly rows [b, e) of the whole pass and batch sizes
do not matter.  Under `process_group=` every rank counts its `search_rows` and the integer rows are gathered in rank order --
moved, never summed -- so every rank ends with the one-process state, bit for bit.

`DC` takes `feature_fn(uint8 images [n, C, H, W] on the device) -> [n, F] array / tensor`, like `PR`."""
import numpy as np
import torch

from .. import dnnlib
from .. import hip_ops
from . import metric_base
from .precision_recall import ManifoldEstimator, _gather_search_rows, _to_device, clamp_batch_sizes, search_rows


def ball_counts_rows(real_features, radii, fake_features, begin, end, row_batch_size, col_batch_size, inclusive=False):
    """Rows [begin, end) of the reals against ALL fakes: how many fakes lie inside each real's balls -> int64
    [end - begin, nk] on the device, exactly those rows of the whole pass.  `radii`: fp64 squared [N, nk], array or tensor.
    The batch sizes are clamped as ManifoldEstimator clamps them.  An empty range launches nothing."""
    real, fake = _to_device(real_features), _to_device(fake_features)
    if fake.shape[1] != real.shape[1]:
        raise ValueError('ball_counts_rows: feature dimension %d of the fakes does not match the reals\' %d' % (fake.shape[1], real.shape[1]))
    radii = torch.as_tensor(radii).to(real.device, torch.float64).contiguous()
    if radii.dim() != 2 or radii.shape[0] != real.shape[0]:
        raise ValueError('ball_counts_rows: radii must be [%d, nk]' % real.shape[0])
    begin, end = int(begin), int(end)
    if not 0 <= begin <= end <= real.shape[0]:
        raise ValueError('ball_counts_rows: need 0 <= begin <= end <= %d' % real.shape[0])
    count = hip_ops.ball_count_state(end - begin, radii.shape[1], real.device)
    if end == begin:
        return count
    row_batch_size, col_batch_size = clamp_batch_sizes(real.shape[1], row_batch_size, col_batch_size)
    fake_norms = hip_ops.row_sqnorm_raw(fake)
    for begin1 in range(begin, end, row_batch_size):
        end1 = min(begin1 + row_batch_size, end)
        rows = real[begin1:end1]
        norms = hip_ops.row_sqnorm_raw(rows)
        for begin2 in range(0, fake.shape[0], col_batch_size):
            end2 = begin2 + col_batch_size
            hip_ops.ball_count_update_raw(rows, norms, radii[begin1:end1], fake[begin2:end2], fake_norms[begin2:end2],
                                          count[begin1 - begin:end1 - begin], inclusive)
    return count


def density_coverage_features(real_features, fake_features, nhood_sizes=[5], row_batch_size=10000, col_batch_size=10000,
                              process_group=None):
    """Density and coverage of two sets of feature vectors; NumPy arrays or device tensors [n, F].  -> EasyDict with
    `radii` fp64 [N, nk] (squared), `counts` int64 [N, nk] (host; kept so that a caller can restrict coverage to a subgroup of
    the reals), `density` [nk] and `coverage` [nk].  `process_group`: every rank of it makes this call with the same two sets,
    runs its `search_rows` of the radius pass and of the count pass and gathers the others'."""
    nhood_sizes = [int(k) for k in nhood_sizes]
    if not nhood_sizes or min(nhood_sizes) < 1:
        raise ValueError('density_coverage_features: neighbourhood sizes must be >= 1 (density divides by k)')
    real, fake = _to_device(real_features), _to_device(fake_features)
    if fake.shape[0] < 1:
        raise ValueError('density_coverage_features: no fakes')
    num_real, num_fake = real.shape[0], fake.shape[0]
    state = dnnlib.EasyDict()
    manifold = ManifoldEstimator(None, real, row_batch_size, col_batch_size, nhood_sizes, process_group=process_group)
    state.radii = manifold.D
    if process_group is None:
        counts = ball_counts_rows(real, state.radii, fake, 0, num_real, row_batch_size, col_batch_size)
    else:
        begin, end = search_rows(num_real, torch.distributed.get_rank(process_group), torch.distributed.get_world_size(process_group))
        own = ball_counts_rows(real, state.radii, fake, begin, end, row_batch_size, col_batch_size)
        counts = _gather_search_rows(own, num_real, process_group)
    state.counts = counts.cpu().numpy().astype(np.int64)
    k_times_m = np.asarray(nhood_sizes, np.int64) * num_fake
    state.density = state.counts.sum(axis=0, dtype=np.int64).astype(np.float64) / k_times_m.astype(np.float64)
    state.coverage = (state.counts > 0).sum(axis=0, dtype=np.int64).astype(np.float64) / np.float64(num_real)
    return state


class DC(metric_base.MetricBase):
    """Under a process group the features of both sets are collected by all ranks (MetricBase._feature_matrix: every rank ends
    with the same [num_images, F] matrices) and the radius and count passes are spread over them by rows."""

    multi_rank = True

    def __init__(self, num_images, nhood_size, minibatch_per_gpu, row_batch_size, col_batch_size, feature_fn=None, **kwargs):
        super().__init__(**kwargs)
        self.num_images = num_images
        self.nhood_size = nhood_size
        self.minibatch_per_gpu = minibatch_per_gpu
        self.row_batch_size = row_batch_size
        self.col_batch_size = col_batch_size
        self.feature_fn = feature_fn
        self._real_features = None

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        if self.feature_fn is None:
            raise RuntimeError('DC needs feature_fn: no feature network ships with this tree')
        if self._real_features is None:      # cached per object
            self._real_features = self._feature_matrix(Gs, Gs_kwargs, 'real', num_gpus)
        fake_features = self._feature_matrix(Gs, Gs_kwargs, 'fake', num_gpus)
        state = density_coverage_features(self._real_features, fake_features, nhood_sizes=[self.nhood_size],
                                          row_batch_size=self.row_batch_size, col_batch_size=self.col_batch_size,
                                          process_group=self._process_group)
        self._report_result(state.density[0], suffix='_density')
        self._report_result(state.coverage[0], suffix='_coverage')
