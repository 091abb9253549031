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


class ManifoldEstimator():
    """Estimate of the manifold of given feature vectors (reference :61-134): one squared radius per point and neighbourhood
    size.  `distance_block` is accepted for the reference's signature and not used (None is fine)."""

    def __init__(self, distance_block, features, row_batch_size, col_batch_size, nhood_sizes, clamp_to_percentile=None):
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
        # The kernels address an operand through 32-bit byte offsets (below 2 GiB each, like DCI.query_chunk / cand_chunk), and the
        # product block of one pass through an int32 element count.
        fit = max(1, 0x7FFFFFF0 // (4 * max(dim, 1)) - 1)
        self.row_batch_size = max(1, min(int(row_batch_size), fit))
        self.col_batch_size = max(1, min(int(col_batch_size), fit, _INT32_MAX // self.row_batch_size))
        self._ref_norms = hip_ops.row_sqnorm_raw(self._ref_features)

        # Squared distance to the k-th neighbour of every point: the kcap = max(nhood) + 1 smallest of its row.
        state = hip_ops.knn_radius_state(num_images, max(self.nhood_sizes) + 1, self._ref_features.device)
        self._fold_radii(state, range(0, num_images, self.col_batch_size))
        self.D = state[:, self.nhood_sizes].cpu().numpy().astype(np.float64)

        if clamp_to_percentile is not None:
            max_distances = np.percentile(self.D, clamp_to_percentile, axis=0)
            self.D[self.D > max_distances] = 0

    def _fold_radii(self, state, col_starts):
        f, n = self._ref_features, self._ref_norms
        for begin1 in range(0, f.shape[0], self.row_batch_size):
            end1 = begin1 + self.row_batch_size
            for begin2 in col_starts:
                end2 = begin2 + self.col_batch_size
                hip_ops.knn_radius_update_raw(f[begin1:end1], n[begin1:end1], f[begin2:end2], n[begin2:end2], state[begin1:end1])

    def evaluate(self, eval_features, return_realism=False, return_neighbors=False):
        """Are new feature vectors in the estimated manifold?  predictions int32 [m, num_nhoods] (+ realism float32 [m], nearest
        reference index int32 [m], in the reference's four return shapes, :127-134)."""
        ev = _to_device(eval_features)
        if ev.shape[1] != self._ref_features.shape[1]:
            raise ValueError('evaluate: feature dimension %d does not match the manifold\'s %d' % (ev.shape[1], self._ref_features.shape[1]))
        dev = ev.device
        num_eval_images, num_ref_images = ev.shape[0], self._ref_features.shape[0]
        radii = torch.from_numpy(np.ascontiguousarray(self.D, dtype=np.float64)).to(dev)
        want_nn = return_realism or return_neighbors
        member = torch.zeros((num_eval_images, self.num_nhoods), device=dev, dtype=torch.int32)
        best_d2, best_idx = hip_ops.nn1_state(num_eval_images, dev)
        for begin1 in range(0, num_eval_images, self.row_batch_size):
            end1 = begin1 + self.row_batch_size
            feature_batch = ev[begin1:end1]
            norms = hip_ops.row_sqnorm_raw(feature_batch)
            for begin2 in range(0, num_ref_images, self.col_batch_size):
                end2 = begin2 + self.col_batch_size
                ref_batch, ref_norms = self._ref_features[begin2:end2], self._ref_norms[begin2:end2]
                hip_ops.manifold_member_update_raw(feature_batch, norms, ref_batch, ref_norms, radii[begin2:end2], member[begin1:end1])
                if want_nn:
                    hip_ops.nn1_update_raw(feature_batch, norms, ref_batch, ref_norms, best_d2[begin1:end1], best_idx[begin1:end1], begin2)
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
                                  row_batch_size=10000, col_batch_size=10000, num_gpus=1):
    """k-NN precision and recall of two sets of feature vectors (reference :138-167); NumPy arrays or device tensors [n, F].
    `feature_net` (the reference reads the feature count off it) and `num_gpus` are accepted for the reference's signature:
    the search runs on the current device, whatever `num_gpus` says."""
    state = dnnlib.EasyDict()
    state.ref_features = _to_device(ref_features)
    state.eval_features = _to_device(eval_features)

    distance_block = DistanceBlock(state.ref_features.shape[1], num_gpus)
    state.ref_manifold = ManifoldEstimator(distance_block, state.ref_features, row_batch_size, col_batch_size, nhood_sizes)
    state.eval_manifold = ManifoldEstimator(distance_block, state.eval_features, row_batch_size, col_batch_size, nhood_sizes)

    # Precision: how many points from eval_features are in the ref_features manifold.
    state.precision, state.realism_scores, state.nearest_neighbors = state.ref_manifold.evaluate(state.eval_features, return_realism=True, return_neighbors=True)
    state.knn_precision = state.precision.mean(axis=0)

    # Recall: how many points from ref_features are in the eval_features manifold.
    state.recall = state.eval_manifold.evaluate(state.ref_features)
    state.knn_recall = state.recall.mean(axis=0)
    return state


class PR(metric_base.MetricBase):
    def __init__(self, num_images, nhood_size, minibatch_per_gpu, row_batch_size, col_batch_size, feature_fn=None, **kwargs):
        super().__init__(**kwargs)
        self.num_images = num_images
        self.nhood_size = nhood_size
        self.minibatch_per_gpu = minibatch_per_gpu
        self.row_batch_size = row_batch_size
        self.col_batch_size = col_batch_size
        self.feature_fn = feature_fn
        self._real_features = None

    def _features(self, images, device):
        f = self.feature_fn(images)
        return torch.as_tensor(f).to(device, torch.float32)          # features stay on the device

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        if self.feature_fn is None:
            raise RuntimeError('PR needs feature_fn: the reference\'s metrics/vgg16.pkl is not available in this tree')
        minibatch_size = num_gpus * self.minibatch_per_gpu

        # Features of the reals, cached per object.
        if self._real_features is None:
            ref_features = None
            for idx, images in enumerate(self._iterate_reals(minibatch_size=minibatch_size)):
                begin = idx * minibatch_size
                end = min(begin + minibatch_size, self.num_images)
                f = self._features(torch.from_numpy(images[:end - begin]).to(Gs.device), Gs.device)
                if ref_features is None:
                    ref_features = torch.empty([self.num_images, f.shape[1]], device=Gs.device, dtype=torch.float32)
                ref_features[begin:end] = f
                if end == self.num_images:
                    break
            self._real_features = ref_features
        ref_features = self._real_features

        # Features of the fakes.
        eval_features = torch.empty_like(ref_features)
        for begin in range(0, self.num_images, minibatch_size):
            end = min(begin + minibatch_size, self.num_images)
            eval_features[begin:end] = self._features(self._generate(Gs, minibatch_size, Gs_kwargs), Gs.device)[:end - begin]

        # Precision and recall (the reference passes row_batch_size for both batch sizes, :219-220).
        state = knn_precision_recall_features(ref_features=ref_features, eval_features=eval_features, nhood_sizes=[self.nhood_size],
                                              row_batch_size=self.row_batch_size, col_batch_size=self.row_batch_size, num_gpus=num_gpus)
        self._report_result(state.knn_precision[0], suffix='_precision')
        self._report_result(state.knn_recall[0], suffix='_recall')
