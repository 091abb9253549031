"""Precision and recall for distributions, PRD (reference: precision-recall-distributions/prd_score.py:48-262; Sajjadi et
al., "Assessing Generative Models via Precision and Recall").  F8 (recall) and F1/8 (precision) of generated against real
embeddings:

    the union of both embeddings is clustered into `num_clusters` bins with mini-batch k-means           (:125-127)
    the two normalised histograms over the bins give the PRD curve at `num_angles` slopes                (:84-103)
    the curves of `num_runs` independent clusterings are averaged                                        (:184-190)
    (F8, F1/8) = the maxima of F_beta and F_1/beta along the curve, beta = 8                             (:260-262)

Everything but the clustering is deterministic NumPy and is the reference's arithmetic, operation by operation.  The
clustering is the random part: the reference uses scikit-learn's MiniBatchKMeans drawn from NumPy's global stream, so its
value is defined in distribution only.  Here the same algorithm runs with every distance, assignment and cluster sum on
the device (csrc/kmeans.hip: the exact distance of the 1-NN and of pr50k3) and every draw from a host
`np.random.RandomState`, so a seed gives one partition:

`minibatch_kmeans(features, num_clusters, n_init, batch_size, max_iter, max_no_improvement, reassignment_ratio, rng)`

    1. a validation subsample of min(3 * batch_size, n) rows is drawn (with replacement);
    2. `n_init` times: k-means++ on the subsample (first centre uniform, every further one with probability proportional
       to the squared distance to the nearest centre so far), one update step on the subsample, then the subsample's
       inertia under the moved centres; the initialisation with the least inertia is kept (the first of equals);
    3. steps on random batches of `batch_size` rows (with replacement), at most max_iter * n // batch_size: rows go to their
       nearest centre, then centre j moves to the running mean  c_j <- (c_j w_j + sum of its rows) / (w_j + count_j),
       w_j <- w_j + count_j.  Master centres are fp64 on the host; the distance step sees their fp32 image, rounded once
       per step;
    4. when some w_j is zero, or 10 * num_clusters rows have gone by since the last check, centres with
       w_j < reassignment_ratio * max w are re-seeded at distinct random rows of the batch (at most batch_size // 2 of
       them) and take the smallest weight among the others;
    5. the batch inertia per row is averaged exponentially (alpha = 2 * batch_size / (n + 1), at most 1); the loop stops
       when the average has not improved for `max_no_improvement` steps;
    6. one step over all rows under the final centres gives the labels.

The reference's cast of the embeddings to fp64 is not made: features stay on the device as fp32 (a network's output is
fp32, and the distances here are exact on those rows).  Non-finite features raise ValueError, as scikit-learn does.
`plot` is not offered (the reference's own script has its call commented out).

The Inception network of the reference (inception.pb) is not available; `PRD` takes
`feature_fn(uint8 images [n, C, H, W] on the device) -> [n, F] array / tensor` instead, like `FID`."""
import numpy as np

from . import metric_base


def compute_prd(eval_dist, ref_dist, num_angles=1001, epsilon=1e-10):
    """PRD curve of the discrete distribution eval_dist with respect to ref_dist on an equiangular grid (reference :48-105)."""
    if not (epsilon > 0 and epsilon < 0.1):
        raise ValueError('epsilon must be in (0, 0.1] but is %s.' % str(epsilon))
    if not (num_angles >= 3 and num_angles <= 1e6):
        raise ValueError('num_angles must be in [3, 1e6] but is %d.' % num_angles)

    angles = np.linspace(epsilon, np.pi/2 - epsilon, num=num_angles)
    slopes = np.tan(angles)
    slopes_2d = np.expand_dims(slopes, 1)
    ref_dist_2d = np.expand_dims(ref_dist, 0)
    eval_dist_2d = np.expand_dims(eval_dist, 0)

    precision = np.minimum(ref_dist_2d*slopes_2d, eval_dist_2d).sum(axis=1)
    recall = precision / slopes

    max_val = max(np.max(precision), np.max(recall))
    if max_val > 1.001:
        raise ValueError('Detected value > 1.001, this should not happen.')
    precision = np.clip(precision, 0, 1)
    recall = np.clip(recall, 0, 1)
    return precision, recall


def _to_device(data):
    from . import precision_recall
    return precision_recall._to_device(data)


def _bins_from_labels(labels, num_eval, num_clusters):
    """The two normalised histograms of the labels of the stacked [eval; ref] rows (reference :129-136)."""
    eval_labels = labels[:num_eval]
    ref_labels = labels[num_eval:]
    eval_bins = np.histogram(eval_labels, bins=num_clusters, range=[0, num_clusters], density=True)[0]
    ref_bins = np.histogram(ref_labels, bins=num_clusters, range=[0, num_clusters], density=True)[0]
    return eval_bins, ref_bins


def minibatch_kmeans(features, num_clusters, n_init=10, batch_size=1024, max_iter=100, max_no_improvement=10,
                     reassignment_ratio=0.01, rng=None):
    """Mini-batch k-means of the rows of `features` [n, dim] (module docstring) -> labels int32 [n] on the host.
    `rng` is a np.random.RandomState (or a seed for one)."""
    import torch
    from .. import hip_ops
    if not isinstance(rng, np.random.RandomState):
        rng = np.random.RandomState(rng)
    X = _to_device(features)
    n, dim = X.shape
    k = int(num_clusters)
    if n < k:
        raise ValueError('n_samples=%d should be >= n_clusters=%d.' % (n, k))
    if not bool(torch.isfinite(X).all()):
        raise ValueError('Input X contains NaN or infinity.')
    dev = X.device
    xnorm = hip_ops.row_sqnorm_raw(X)
    batch_size = min(int(batch_size), n)

    def step(rows, rnorm, centres64):
        """-> d2 [m], sums [k', dim], count [k'], inertia on the host (fp64 / int64), under the fp32 image of the centres."""
        c32 = torch.from_numpy(np.ascontiguousarray(centres64, dtype=np.float32)).to(dev)
        _, d2, sums, count, inertia = hip_ops.kmeans_step(rows, rnorm, c32)
        return d2, sums.cpu().numpy(), count.cpu().numpy(), float(inertia.cpu().numpy()[0])

    def gather(idx):
        i = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev)
        return X.index_select(0, i), xnorm.index_select(0, i)

    def move(centres, weights, sums, count):
        hit = count > 0
        total = weights[hit] + count[hit]
        centres[hit] = (centres[hit] * weights[hit, None] + sums[hit]) / total[:, None]
        weights[hit] = total

    # 1. validation subsample
    valid_idx = rng.randint(0, n, size=min(3 * batch_size, n))
    Xv, vnorm = gather(valid_idx)
    nv = Xv.shape[0]

    # 2. the best of n_init k-means++ initialisations
    best = None
    for _ in range(int(n_init)):
        chosen = [int(rng.randint(nv))]
        closest = None
        for _c in range(1, k):
            d2, _, _, _ = step(Xv, vnorm, Xv[chosen[-1]:chosen[-1] + 1].double().cpu().numpy())
            d2 = d2.cpu().numpy()
            closest = d2 if closest is None else np.minimum(closest, d2)
            cum = np.cumsum(closest)
            pick = int(np.searchsorted(cum, rng.random_sample() * cum[-1]))
            chosen.append(min(pick, nv - 1))
        centres = Xv.index_select(0, torch.as_tensor(chosen, device=dev)).double().cpu().numpy()
        weights = np.zeros(k, np.float64)
        _, sums, count, _ = step(Xv, vnorm, centres)
        move(centres, weights, sums, count)
        _, _, _, inertia = step(Xv, vnorm, centres)
        if best is None or inertia < best[0]:
            best = (inertia, centres, weights)
    _, centres, weights = best

    # 3. - 5. steps on random batches
    n_steps = (int(max_iter) * n) // batch_size
    alpha = min(batch_size * 2.0 / (n + 1), 1.0)
    ewa = ewa_min = None
    no_improvement = 0
    since_reassign = 0
    for _ in range(n_steps):
        idx = rng.randint(0, n, size=batch_size)
        Xb, bnorm = gather(idx)
        _, sums, count, inertia = step(Xb, bnorm, centres)
        move(centres, weights, sums, count)
        since_reassign += batch_size
        if (weights == 0).any() or since_reassign >= 10 * k:
            since_reassign = 0
            to_reassign = weights < reassignment_ratio * weights.max()
            if to_reassign.sum() > batch_size // 2:
                keep = np.argsort(weights, kind='stable')[batch_size // 2:]
                to_reassign[keep] = False
            n_reassign = int(to_reassign.sum())
            if n_reassign:
                rows = rng.choice(batch_size, replace=False, size=n_reassign)
                centres[to_reassign] = Xb.index_select(0, torch.from_numpy(rows.astype(np.int64)).to(dev)).double().cpu().numpy()
                weights[to_reassign] = np.min(weights[~to_reassign])
        per_row = inertia / batch_size
        ewa = per_row if ewa is None else ewa * (1.0 - alpha) + per_row * alpha
        if ewa_min is None or ewa < ewa_min:
            ewa_min = ewa
            no_improvement = 0
        else:
            no_improvement += 1
        if max_no_improvement is not None and no_improvement >= max_no_improvement:
            break

    # 6. labels of all rows
    c32 = torch.from_numpy(np.ascontiguousarray(centres, dtype=np.float32)).to(dev)
    label, _, _, _, _ = hip_ops.kmeans_step(X, xnorm, c32)
    return label.cpu().numpy()


def _cluster_into_bins(eval_data, ref_data, num_clusters, rng=None):
    """Clusters the union of the data points and returns the cluster distribution (reference :108-136)."""
    import torch
    eval_data, ref_data = _to_device(eval_data), _to_device(ref_data)
    cluster_data = torch.cat([eval_data, ref_data])
    labels = minibatch_kmeans(cluster_data, num_clusters, n_init=10, rng=rng)
    return _bins_from_labels(labels, len(eval_data), num_clusters)


def compute_prd_from_embedding(eval_data, ref_data, num_clusters=20, num_angles=1001, num_runs=10, enforce_balance=False,
                               seed=None):
    """PRD curve of two sample embeddings, averaged over `num_runs` clusterings (reference :139-191).  `seed` seeds the one
    RandomState all runs draw from (None: a fresh unseeded one; NumPy's global stream is never touched)."""
    if enforce_balance and len(eval_data) != len(ref_data):
        raise ValueError(
            'The number of points in eval_data %d is not equal to the number of '
            'points in ref_data %d. To disable this exception, set enforce_balance '
            'to False (not recommended).' % (len(eval_data), len(ref_data)))

    rng = np.random.RandomState(seed)
    eval_data, ref_data = _to_device(eval_data), _to_device(ref_data)
    precisions = []
    recalls = []
    for _ in range(num_runs):
        eval_dist, ref_dist = _cluster_into_bins(eval_data, ref_data, num_clusters, rng=rng)
        precision, recall = compute_prd(eval_dist, ref_dist, num_angles)
        precisions.append(precision)
        recalls.append(recall)
    precision = np.mean(precisions, axis=0)
    recall = np.mean(recalls, axis=0)
    return precision, recall


def _prd_to_f_beta(precision, recall, beta=1, epsilon=1e-10):
    """F_beta scores of precision / recall pairs (reference :194-227)."""
    if not ((precision >= 0).all() and (precision <= 1).all()):
        raise ValueError('All values in precision must be in [0, 1].')
    if not ((recall >= 0).all() and (recall <= 1).all()):
        raise ValueError('All values in recall must be in [0, 1].')
    if beta <= 0:
        raise ValueError('Given parameter beta %s must be positive.' % str(beta))

    return (1 + beta**2) * (precision * recall) / (
        (beta**2 * precision) + recall + epsilon)


def prd_to_max_f_beta_pair(precision, recall, beta=8):
    """(max F_beta, max F_1/beta) along a PRD curve (reference :230-262)."""
    if not ((precision >= 0).all() and (precision <= 1).all()):
        raise ValueError('All values in precision must be in [0, 1].')
    if not ((recall >= 0).all() and (recall <= 1).all()):
        raise ValueError('All values in recall must be in [0, 1].')
    if beta <= 0:
        raise ValueError('Given parameter beta %s must be positive.' % str(beta))

    f_beta = np.max(_prd_to_f_beta(precision, recall, beta))
    f_beta_inv = np.max(_prd_to_f_beta(precision, recall, 1/beta))
    return f_beta, f_beta_inv


class PRD(metric_base.MetricBase):
    """Under a process group the features of both sets are collected by all ranks (MetricBase._feature_matrix) and
    every rank ends with the same two matrices in the same row order.  The clustering depends on that order and on one seeded
    RandomState, so every rank runs it and gets the same numbers; nothing is broadcast from rank 0."""

    multi_rank = True

    def __init__(self, num_images, num_clusters, num_angles, num_runs, minibatch_per_gpu, feature_fn=None, seed=0, **kwargs):
        super().__init__(**kwargs)
        self.num_images = num_images
        self.num_clusters = num_clusters
        self.num_angles = num_angles
        self.num_runs = num_runs
        self.minibatch_per_gpu = minibatch_per_gpu
        self.feature_fn = feature_fn
        self.seed = seed
        self._real_features = None

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        if self.feature_fn is None:
            raise RuntimeError('PRD needs feature_fn: the reference\'s precision-recall-distributions/inception.pb is not available in this tree')
        if self._real_features is None:      # cached per object
            self._real_features = self._feature_matrix(Gs, Gs_kwargs, 'real', num_gpus)
        ref_features = self._real_features
        eval_features = self._feature_matrix(Gs, Gs_kwargs, 'fake', num_gpus)

        precision, recall = compute_prd_from_embedding(eval_features, ref_features, num_clusters=self.num_clusters,
                                                       num_angles=self.num_angles, num_runs=self.num_runs, seed=self.seed)
        f_beta, f_beta_inv = prd_to_max_f_beta_pair(precision, recall, beta=8)
        self._report_result(f_beta, suffix='_F8')
        self._report_result(f_beta_inv, suffix='_F1_8')
