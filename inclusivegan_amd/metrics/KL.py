"""KL divergence of the generated Stacked-MNIST class histogram from the uniform distribution (reference: metrics/KL.py:20-52):
    density_fake = histogram(labels, bins = 0..K, density=True);  KL = sum_{p > 0} p * log(p / (1 / K)).
Classifier injected, or picked up from `classifier_pkl`, as in mode_counts; float32 device logits are folded into a class histogram on the device and the
divergence is taken from the K counts (`kl_from_counts`, bit for bit `kl_to_uniform` of the labels behind them).  Under a
process group every rank folds its share and the counts are summed exactly (mode_counts.merged_class_counts)."""
import numpy as np

from . import metric_base
from .mode_counts import DEFAULT_CLASSIFIER_PKL, class_statistics, merged_class_counts, predicted_labels  # noqa: F401  (predicted_labels: the host statement, kept importable)


def kl_to_uniform(labels_all, num_classes):
    density_fake = np.histogram(labels_all, bins=np.arange(num_classes + 1), density=True)[0]
    density_real = np.ones(num_classes, dtype=np.float32) / float(num_classes)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.sum(np.where(density_fake != 0, density_fake * np.log(density_fake / density_real), 0))


def kl_from_counts(counts):
    """kl_to_uniform from the class histogram instead of the labels: the density is counts / (bin width 1.0) / counts.sum(),
    as np.histogram(density=True) computes it, then the same statement."""
    counts = np.asarray(counts)
    num_classes = counts.shape[0]
    with np.errstate(divide='ignore', invalid='ignore'):
        density_fake = counts / np.ones(num_classes, dtype=float) / counts.sum()
        density_real = np.ones(num_classes, dtype=np.float32) / float(num_classes)
        return np.sum(np.where(density_fake != 0, density_fake * np.log(density_fake / density_real), 0))


class KL(metric_base.MetricBase):
    multi_rank = True

    def __init__(self, num_images, minibatch_per_gpu, classify_fn=None, classifier_pkl=DEFAULT_CLASSIFIER_PKL, **kwargs):
        super().__init__(**kwargs)
        self.num_images = num_images
        self.minibatch_per_gpu = minibatch_per_gpu
        self.classify_fn = classify_fn
        self.classifier_pkl = classifier_pkl

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        import torch
        if self._process_group is not None:
            counts = merged_class_counts(self, Gs, Gs_kwargs)
            if torch.distributed.get_rank(self._process_group) == 0:
                self._report_result(kl_from_counts(counts))
            return
        counts, labels_all, num_classes = class_statistics(self, Gs, Gs_kwargs, num_gpus)
        self._report_result(kl_from_counts(counts) if counts is not None else kl_to_uniform(labels_all, num_classes))
