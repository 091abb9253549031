"""k-NN precision and recall (reference: metrics/precision_recall.py:20-222; Kynkaanniemi et al., "Improved Precision and
Recall Metric for Assessing Generative Models").

    radius of a point, neighbourhood k = the value at 0-based position k of its ascending squared distances to ALL points of
                                         its own set, itself included (np.partition(...)[:, nhood_sizes], :76,90)
    a sample is in the manifold        = some point of the set has d2(sample, point) <= radius(point)          (:119-120)
    precision = share of fakes in the manifold of the reals; recall = share of reals in the manifold of the fakes  (:156-162)
    realism = radius(nearest, nhood_sizes[0]) / min d2, squared over squared                                     (:124-125)

The reference fills [10 000 x n] float16 distance blocks on the GPUs and partitions them on the host.  Here the search is
the exact streaming one of the 1-NN (csrc/exact_search.hip): the fp32 MFMA product only screens, every pair it
cannot decide is measured as a direct difference in fp64, so radii, predictions and nearest indices equal an fp64 brute
force on the same fp32 features; nothing larger than one product block exists and nothing but the results visits the host.
`.D` therefore holds float64 SQUARED radii (the reference: float16).

Every state of the search is a function of the set of (row, index) pairs fed to it, so rows [b, e) of a pass against all
columns are exactly rows [b, e) of the whole pass: `ManifoldEstimator.radii_rows` / `evaluate_rows` run a row range, and under
`process_group=` every rank runs its `search_rows` of each pass and the results are gathered in rank order, which is row
order.  Every rank passes the same feature sets and ends with the one-process state, bit for bit.

The VGG-16 feature network of the reference (metrics/vgg16.pkl) is not available; `PR` takes
`feature_fn(uint8 images [n, C, H, W] on the device) -> [n, F] array / tensor` instead, like `FID`."""
import numpy as np
import torch

from .. import dnnlib
from .. import hip_ops
from . import metric_base

_INT32_MAX = 2 ** 31 - 1


def batch_pairwise_distances(U, V):
    """Pairwise squared distances of two feature batches in the clamped cancellation form (reference :20-34), fp32 on the
    device.  Kept for callers of the reference's surface; the estimator below does not use it."""
    U = torch.as_tensor(U, dtype=torch.float32)
    V = torch.as_tensor(V, dtype=torch.float32).to(U.device)
    norm_u = torch.sum(torch.square(U), 1).reshape(-1, 1)
    norm_v = torch.sum(torch.square(V), 1).reshape(1, -1)
    return torch.clamp(norm_u - 2 * torch.matmul(U, V.t()) + norm_v, min=0.0)


class DistanceBlock():
    """Distance block (reference :38-57).  `num_gpus` is accepted; the block is computed on the current device."""

    def __init__(self, num_features, num_gpus):
        self.num_features = num_features
        self.num_gpus = num_gpus

    def pairwise_distances(self, U, V):
        dev = torch.device('cuda', torch.cuda.current_device())
        U = torch.as_tensor(U, dtype=torch.float32).to(dev)
        V = torch.as_tensor(V, dtype=torch.float32).to(dev)
        return batch_pairwise_distances(U, V).cpu().numpy()


def _to_device(features):
    """NumPy array or tensor [n, F] -> contiguous fp32 tensor on the current ROCm device (host arrays are moved in 64 MB pieces)."""
    if not torch.cuda.is_available():
        raise RuntimeError('inclusivegan_amd precision / recall needs a ROCm device; there is no CPU path')
    dev = torch.device('cuda', torch.cuda.current_device())
    if torch.is_tensor(features):
        if features.dim() != 2:
            raise ValueError('features must be [n, F]')
        return features.to(dev, torch.float32).contiguous()
    arr = np.asarray(features)
    if arr.ndim != 2:
        raise ValueError('features must be [n, F]')
    out = torch.empty(arr.shape, device=dev, dtype=torch.float32)
    step = max(1, (64 << 20) // (4 * max(arr.shape[1], 1)))
    for i in range(0, arr.shape[0], step):
        out[i:i + step] = torch.from_numpy(np.ascontiguousarray(arr[i:i + step], dtype=np.float32)).to(dev)
    return out


def search_rows(n, rank, world):
    """The rows [begin, end) of an n-row search that rank `rank` of `world` runs: over the ranks the ranges are disjoint, in
    rank order, cover [0, n), differ in length by at most one and may be empty."""
    n, rank, world = int(n), int(rank), int(world)
    if n < 0 or world < 1 or not 0 <= rank < world:
        raise ValueError('search_rows: need n >= 0 and 0 <= rank < world')
    return rank * n // world, (rank + 1) * n // world


def _gather_search_rows(own, n, group):
    """Every rank's `search_rows` slice of an n-row result -> all n rows on every rank, in rank order, which is row order."""
    world = torch.distributed.get_world_size(group)
    out = torch.empty((n,) + tuple(own.shape[1:]), device=own.device, dtype=own.dtype)
    return metric_base.gather_rows(out, [[search_rows(n, r, world)] for r in range(world)], own, group)


def clamp_batch_sizes(dim, row_batch_size, col_batch_size):
    """(row, col) batch sizes a search pass can use: the kernels address an operand through 32-bit byte offsets (below 2 GiB each,
    like DCI.query_chunk / cand_chunk), and the product block of one pass through an int32 element count."""
    fit = max(1, 0x7FFFFFF0 // (4 * max(dim, 1)) - 1)
    row_batch_size = max(1, min(int(row_batch_size), fit))
    return row_batch_size, max(1, min(int(col_batch_size), fit, _INT32_MAX // row_batch_size))


class ManifoldEstimator():
    """Estimate of the manifold of given feature vectors (reference :61-134): one squared radius per point and neighbourhood
    size.  `distance_block` is accepted for the reference's signature and not used (None is fine)."""

    def __init__(self, distance_block, features, row_batch_size, col_batch_size, nhood_sizes, clamp_to_percentile=None,
                 process_group=None):
        self._process_group = process_group
        self.nhood_sizes = [int(k) for k in nhood_sizes]
        self.num_nhoods = len(self.nhood_sizes)
        self._distance_block = distance_block
        self._ref_features = _to_device(features)
        num_images, dim = self._ref_features.shape
        if self.num_nhoods < 1 or min(self.nhood_sizes) < 0:
            raise ValueError('nhood_sizes must hold at least one non-negative neighbourhood size')
        if num_images <= max(self.nhood_sizes):
            raise ValueError('ManifoldEstimator: %d points cannot have a neighbour at position %d' % (num_images, max(self.nhood_sizes)))
        if max(self.nhood_sizes) + 1 > 16 or self.num_nhoods > 8:
            raise ValueError('ManifoldEstimator: the HIP search keeps at most 16 distances per point (nhood sizes <= 15) and 8 neighbourhood sizes')
        self.row_batch_size, self.col_batch_size = clamp_batch_sizes(dim, row_batch_size, col_batch_size)
        self._ref_norms = hip_ops.row_sqnorm_raw(self._ref_features)

        # Squared distance to the k-th neighbour of every point: the kcap = max(nhood) + 1 smallest of its row.
        if process_group is None:
            radii = self.radii_rows(0, num_images)
        else:   # every rank its rows; all of them are in place before any membership pass needs a column's radius
            radii = self.radii_rows(*search_rows(num_images, torch.distributed.get_rank(process_group), torch.distributed.get_world_size(process_group)))
            radii = _gather_search_rows(radii, num_images, process_group)
        self.D = radii.cpu().numpy().astype(np.float64)

        if clamp_to_percentile is not None:
            max_distances = np.percentile(self.D, clamp_to_percentile, axis=0)
            self.D[self.D > max_distances] = 0

    def radii_rows(self, begin, end):
        """The squared radii of rows [begin, end) of the feature set against ALL of it -> fp64 [end - begin, num_nhoods] on the
        device: exactly those rows of the whole search (a row's state is a function of the set of columns fed to it).  An
        empty range launches nothing."""
        f, n = self._ref_features, self._ref_norms
        begin, end = int(begin), int(end)
        if not 0 <= begin <= end <= f.shape[0]:
            raise ValueError('radii_rows: need 0 <= begin <= end <= %d' % f.shape[0])
        state = hip_ops.knn_radius_state(end - begin, max(self.nhood_sizes) + 1, f.device)
        for begin1 in range(begin, end, self.row_batch_size):
            end1 = min(begin1 + self.row_batch_size, end)
            for begin2 in range(0, f.shape[0], self.col_batch_size):
                end2 = begin2 + self.col_batch_size
                hip_ops.knn_radius_update_raw(f[begin1:end1], n[begin1:end1], f[begin2:end2], n[begin2:end2], state[begin1 - begin:end1 - begin])
        return state[:, self.nhood_sizes].contiguous()

    def evaluate_rows(self, eval_features, begin, end, want_nn=False):
        """Rows [begin, end) of `eval_features` against all reference rows and all radii -> (member int32 [end - begin,
        num_nhoods], best_d2 fp64 [end - begin], best_idx int32 [end - begin]) on the device, the two last in their initial
        state (+inf, INT32_MAX) without `want_nn`: exactly those rows of the whole evaluation.  With `want_nn` membership and
        nearest neighbour share one product block (igan_manifold_member_nn1_update).  An empty range launches nothing."""
        ev = _to_device(eval_features)
        if ev.shape[1] != self._ref_features.shape[1]:
            raise ValueError('evaluate: feature dimension %d does not match the manifold\'s %d' % (ev.shape[1], self._ref_features.shape[1]))
        begin, end = int(begin), int(end)
        if not 0 <= begin <= end <= ev.shape[0]:
            raise ValueError('evaluate_rows: need 0 <= begin <= end <= %d' % ev.shape[0])
        dev = ev.device
        num_ref_images = self._ref_features.shape[0]
        radii = torch.from_numpy(np.ascontiguousarray(self.D, dtype=np.float64)).to(dev)
        member = torch.zeros((end - begin, self.num_nhoods), device=dev, dtype=torch.int32)
        best_d2, best_idx = hip_ops.nn1_state(end - begin, dev)
        for begin1 in range(begin, end, self.row_batch_size):
            end1 = min(begin1 + self.row_batch_size, end)
            rows = slice(begin1 - begin, end1 - begin)
            feature_batch = ev[begin1:end1]
            norms = hip_ops.row_sqnorm_raw(feature_batch)
            for begin2 in range(0, num_ref_images, self.col_batch_size):
                end2 = begin2 + self.col_batch_size
                ref_batch, ref_norms = self._ref_features[begin2:end2], self._ref_norms[begin2:end2]
                if want_nn:
                    hip_ops.manifold_member_nn1_update_raw(feature_batch, norms, ref_batch, ref_norms, radii[begin2:end2], member[rows],
                                                           best_d2[rows], best_idx[rows], begin2)
                else:
                    hip_ops.manifold_member_update_raw(feature_batch, norms, ref_batch, ref_norms, radii[begin2:end2], member[rows])
        return member, best_d2, best_idx

    def evaluate(self, eval_features, return_realism=False, return_neighbors=False):
        """Are new feature vectors in the estimated manifold?  predictions int32 [m, num_nhoods] (+ realism float32 [m], nearest
        reference index int32 [m], in the reference's four return shapes, :127-134).  Under the estimator's process group
        every rank passes the same `eval_features`, searches its `search_rows` and ends with all rows."""
        ev = _to_device(eval_features)
        want_nn = return_realism or return_neighbors
        group = self._process_group
        if group is None:
            member, best_d2, best_idx = self.evaluate_rows(ev, 0, ev.shape[0], want_nn)
        else:
            own = search_rows(ev.shape[0], torch.distributed.get_rank(group), torch.distributed.get_world_size(group))
            member, best_d2, best_idx = self.evaluate_rows(ev, own[0], own[1], want_nn)
            member = _gather_search_rows(member, ev.shape[0], group)
            if want_nn:
                best_d2, best_idx = _gather_search_rows(best_d2, ev.shape[0], group), _gather_search_rows(best_idx, ev.shape[0], group)
        return self.evaluation_results(member, best_d2, best_idx, return_realism, return_neighbors)

    def evaluation_results(self, member, best_d2, best_idx, return_realism=False, return_neighbors=False):
        """The host statements on the device state of all rows (`evaluate_rows`, or its row ranges concatenated in row order)
        -> what `evaluate` returns."""
        want_nn = return_realism or return_neighbors
        batch_predictions = member.cpu().numpy().astype(np.int32)
        if not want_nn:
            return batch_predictions
        # a sample with no finite distance at all (a NaN row) has every distance +inf: the arg-min of equal values is index 0
        nearest_indices = torch.where(best_idx == _INT32_MAX, torch.zeros_like(best_idx), best_idx).cpu().numpy().astype(np.int32)
        with np.errstate(divide='ignore', invalid='ignore'):
            realism_score = (self.D[nearest_indices, 0] / best_d2.cpu().numpy()).astype(np.float32)

        if return_realism and return_neighbors:
            return batch_predictions, realism_score, nearest_indices
        elif return_realism:
            return batch_predictions, realism_score
        return batch_predictions, nearest_indices


def knn_precision_recall_features(ref_features, eval_features, feature_net=None, nhood_sizes=[3],
                                  row_batch_size=10000, col_batch_size=10000, num_gpus=1, process_group=None):
    """k-NN precision and recall of two sets of feature vectors (reference :138-167); NumPy arrays or device tensors [n, F].
    `feature_net` (the reference reads the feature count off it) and `num_gpus` are accepted for the reference's signature:
    the search runs on the current device, whatever `num_gpus` says.  `process_group`: every rank of it makes this call with
    the same two feature sets, searches its `search_rows` of each of the four passes (two radii, two memberships) and
    gathers the others', so every rank returns the state of the one-process call, bit for bit."""
    state = dnnlib.EasyDict()
    state.ref_features = _to_device(ref_features)
    state.eval_features = _to_device(eval_features)

    distance_block = DistanceBlock(state.ref_features.shape[1], num_gpus)
    state.ref_manifold = ManifoldEstimator(distance_block, state.ref_features, row_batch_size, col_batch_size, nhood_sizes, process_group=process_group)
    state.eval_manifold = ManifoldEstimator(distance_block, state.eval_features, row_batch_size, col_batch_size, nhood_sizes, process_group=process_group)

    # Precision: how many points from eval_features are in the ref_features manifold.
    state.precision, state.realism_scores, state.nearest_neighbors = state.ref_manifold.evaluate(state.eval_features, return_realism=True, return_neighbors=True)
    state.knn_precision = state.precision.mean(axis=0)

    # Recall: how many points from ref_features are in the eval_features manifold.
    state.recall = state.eval_manifold.evaluate(state.ref_features)
    state.knn_recall = state.recall.mean(axis=0)
    return state


class PR(metric_base.MetricBase):
    """Under a process group the features of both sets are collected by all ranks (MetricBase._feature_matrix: every rank
    ends with the same [num_images, F] matrices) and the four passes of the search are spread over them by rows."""

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
            raise RuntimeError('PR needs feature_fn: the reference\'s metrics/vgg16.pkl is not available in this tree')
        if self._real_features is None:      # cached per object
            self._real_features = self._feature_matrix(Gs, Gs_kwargs, 'real', num_gpus)
        ref_features = self._real_features
        eval_features = self._feature_matrix(Gs, Gs_kwargs, 'fake', num_gpus)

        # Precision and recall (the reference passes row_batch_size for both batch sizes, :219-220).
        state = knn_precision_recall_features(ref_features=ref_features, eval_features=eval_features, nhood_sizes=[self.nhood_size],
                                              row_batch_size=self.row_batch_size, col_batch_size=self.row_batch_size, num_gpus=num_gpus,
                                              process_group=self._process_group)
        self._report_result(state.knn_precision[0], suffix='_precision')
        self._report_result(state.knn_recall[0], suffix='_recall')
