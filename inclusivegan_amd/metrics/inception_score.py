"""Inception Score (reference: metrics/inception_score.py:18-56; Salimans et al., "Improved Techniques for Training GANs").

    per split: exp(mean over images of KL(p(y | x) || p(y))), p(y) the split's own mean; reported: mean and std over splits

The Inception-v3 softmax network of the reference (metrics/inception_v3_softmax.pkl) is not available; `IS` takes
`classify_fn(uint8 images [n, C, H, W] on the device) -> softmax probabilities [n, K]` instead, like `FID`'s `feature_fn`.
Probabilities that come back as device tensors stay on the device: every minibatch is cast to float32 as the host path
casts it and folded into a `hip_ops.SplitProbStats` (csrc/class_stats.hip: per split the row count, the fp64 column sums and the
fp64 sum of p log p, in a fixed order), and a split's score is  exp(plogp / n - sum_k m_k log m_k),  m = psum / n  -- the
reference's statement with the mean over the images taken first.  NumPy / CPU results are collected on the host and go
through the reference's statement, value for value.

Under a process group (`run(..., process_group=)`) the images are dealt to the ranks (`MetricBase._walk`); a row's split is
decided by its GLOBAL index, every rank folds its rows,
`SplitProbStats.all_merge` leaves every rank with the same bits and rank 0 reports.  Host results are REFUSED under a group."""
import numpy as np
import torch

from .. import hip_ops
from . import metric_base


def inception_score_splits(activations, num_splits):
    """exp(mean KL) of every split of float32 probabilities [n, K]; split i holds rows i * n // num_splits .. (i + 1) * n //
    num_splits, so the splits differ in size when num_splits does not divide n (:50-54)."""
    num_images = activations.shape[0]
    scores = []
    for i in range(num_splits):
        part = activations[i * num_images // num_splits: (i + 1) * num_images // num_splits]
        kl = part * (np.log(part) - np.log(np.expand_dims(np.mean(part, 0), 0)))
        kl = np.mean(np.sum(kl, 1))
        scores.append(np.exp(kl))
    return scores


class IS(metric_base.MetricBase):
    multi_rank = True

    def __init__(self, num_images, num_splits, minibatch_per_gpu, classify_fn=None, **kwargs):
        super().__init__(**kwargs)
        self.num_images = num_images
        self.num_splits = num_splits
        self.minibatch_per_gpu = minibatch_per_gpu
        self.classify_fn = classify_fn

    def _folded(self, stats, begin, probs):
        """`stats` (None: a new hip_ops.SplitProbStats) with one minibatch of device probabilities folded in, cast to float32 as
        the host path casts it."""
        if stats is None:
            stats = hip_ops.SplitProbStats(probs.shape[1], self.num_images, self.num_splits, probs.device)
        stats.update(probs.detach().to(torch.float32), begin)
        return stats

    def _shard_stats(self, Gs, Gs_kwargs, rank, world):
        """hip_ops.SplitProbStats of the fakes rank `rank` of `world` owns, or None when it owns none -- a function of its
        arguments alone (MetricBase._walk), so one process can rebuild every rank's state."""
        stats = None

        def fold(begin, end, probs):
            nonlocal stats
            stats = self._folded(stats, begin, self._device_result(probs, 'classify_fn'))

        self._walk(Gs, Gs_kwargs, 'fake', self.classify_fn, fold, 'images', shard=(rank, world))
        return stats

    def _evaluate_sharded(self, Gs, Gs_kwargs):
        group = self._process_group
        rank, world = torch.distributed.get_rank(group), torch.distributed.get_world_size(group)
        stats = self._shard_stats(Gs, Gs_kwargs, rank, world)
        K = self._agree_on_width(stats.K if stats is not None else 0, Gs.device, 'probability')
        if stats is None:
            stats = hip_ops.SplitProbStats(K, self.num_images, self.num_splits, Gs.device)
        scores = stats.all_merge(group).scores()
        if rank == 0:
            self._report_result(np.mean(scores), suffix='_mean')
            self._report_result(np.std(scores), suffix='_std')

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        if self.classify_fn is None:
            raise RuntimeError('IS needs classify_fn: the reference\'s metrics/inception_v3_softmax.pkl is not available in this tree')
        if self._process_group is not None:
            return self._evaluate_sharded(Gs, Gs_kwargs)
        activations = stats = None

        # Calculate activations for fakes.
        def fold(begin, end, probs):
            nonlocal activations, stats
            on_device = torch.is_tensor(probs) and probs.is_cuda
            self._same_kind(begin == 0, on_device, stats is not None, 'classify_fn')
            if on_device:
                stats = self._folded(stats, begin, probs)
                return
            probs = torch.as_tensor(probs).detach().to('cpu', torch.float32).numpy()
            if activations is None:
                activations = np.empty([self.num_images, probs.shape[1]], dtype=np.float32)
            activations[begin:end] = probs

        self._walk(Gs, Gs_kwargs, 'fake', self.classify_fn, fold, 'result', num_gpus=num_gpus)

        # Calculate IS.
        scores = stats.scores() if stats is not None else inception_score_splits(activations, self.num_splits)
        self._report_result(np.mean(scores), suffix='_mean')
        self._report_result(np.std(scores), suffix='_std')
