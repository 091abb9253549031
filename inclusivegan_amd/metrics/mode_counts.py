"""Number of Stacked-MNIST modes covered by the generator (reference: metrics/mode_counts.py:20-49): classify `num_images`
fakes into the 1000 digit triples and count the distinct classes hit.  The classifier (metrics/stacked_mnist_classifier.pkl
in the reference) is injected: `classify_fn(float images [n, C, H, W] in [-1, 1]) -> logits [n, K]`; without one, the pickle
this project's own trainer wrote at `classifier_pkl` (train_classifier.py, the reference's path by default) is picked up.

Logits that come back as float32 device tensors stay on the device: every minibatch is folded into a
`hip_ops.ClassHistogram` (csrc/class_stats.hip: np.argmax per row, 64-bit integer counts) and the K counts are the one device
-> host copy; the mode count and KL.py's divergence are functions of the counts (`count_modes_from_counts`,
`KL.kl_from_counts`).  Any other result -- NumPy, a CPU tensor, another dtype -- goes through np.argmax on the host, the
reference's statements.

Under a process group (`run(..., process_group=)`) the images are dealt to the ranks (`MetricBase._walk`), every rank folds
its rows into its own histogram, one all_reduce(SUM) of the int64 counts gives every rank the exact total and rank 0 reports.
Host results are REFUSED under a group: they are evaluated by one process."""
import numpy as np

from . import metric_base


DEFAULT_CLASSIFIER_PKL = 'metrics/stacked_mnist_classifier.pkl'      # the reference's path (:29), relative to the working directory


def _resolve_classifier(metric):
    """An injected classify_fn always wins; without one, the pickle train_classifier wrote at metric.classifier_pkl is loaded
    (once per metric object); without either, the error."""
    import os
    if metric.classify_fn is not None:
        return
    pkl = getattr(metric, 'classifier_pkl', None)
    if pkl and os.path.isfile(pkl):
        from ..train_classifier import load_classify_fn
        metric.classify_fn = load_classify_fn(pkl)
        return
    raise RuntimeError('%s needs classify_fn: the reference\'s metrics/stacked_mnist_classifier.pkl is not available in this tree. '
                       'Train this project\'s own classifier with `python -m inclusivegan_amd.train_classifier`.' % metric.name)


def _host(logits):
    import torch
    return logits.detach().cpu().numpy() if torch.is_tensor(logits) else np.asarray(logits)


def predicted_labels(metric, Gs, Gs_kwargs, num_gpus):
    _resolve_classifier(metric)
    labels_all = np.empty([metric.num_images], dtype=np.float32)
    num_classes = None

    def fold(begin, end, logits):
        nonlocal num_classes
        num_classes = logits.shape[1]
        labels_all[begin:end] = np.argmax(_host(logits), axis=1)

    metric._walk(Gs, Gs_kwargs, 'fake', metric.classify_fn, fold, 'result', num_gpus=num_gpus, as_uint8=False)     # the classifier sees G's float output (:39-40)
    return labels_all, num_classes


def count_modes(labels_all):
    return len(np.unique(labels_all))


def counts_of_labels(labels_all, num_classes):
    """The class histogram KL.kl_to_uniform takes of the labels (np.histogram over the bins 0 .. K)."""
    return np.histogram(labels_all, bins=np.arange(num_classes + 1))[0]


def count_modes_from_counts(counts):
    return int(np.count_nonzero(counts))


def _on_device_f32(logits):
    import torch
    return torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32


def class_statistics(metric, Gs, Gs_kwargs, num_gpus):
    """One process, the draws of `predicted_labels`: float32 device logits are folded on the device -> (counts [K] NumPy
    integers, None, K); anything else is labelled on the host as there -> (None, labels_all, K)."""
    from .. import hip_ops
    _resolve_classifier(metric)
    hist = labels_all = num_classes = None

    def fold(begin, end, logits):
        nonlocal hist, labels_all, num_classes
        on_device = _on_device_f32(logits)
        metric._same_kind(begin == 0, on_device, hist is not None, 'classify_fn', 'float32 device tensors')
        if on_device:
            if hist is None:
                hist = hip_ops.ClassHistogram(logits.shape[1], logits.device)
            hist.update(logits)
        else:
            if labels_all is None:
                labels_all = np.empty([metric.num_images], dtype=np.float32)
            num_classes = logits.shape[1]
            labels_all[begin:end] = np.argmax(_host(logits), axis=1)

    metric._walk(Gs, Gs_kwargs, 'fake', metric.classify_fn, fold, 'result', num_gpus=num_gpus, as_uint8=False)     # the classifier sees G's float output (:39-40)
    return (hist.to_host(), None, hist.K) if hist is not None else (None, labels_all, num_classes)


def shard_histogram(metric, Gs, Gs_kwargs, rank, world):
    """hip_ops.ClassHistogram of the fakes rank `rank` of `world` owns, or None when it owns none -- a function of its
    arguments alone (MetricBase._walk), so one process can rebuild every rank's state."""
    import torch
    from .. import hip_ops
    _resolve_classifier(metric)
    hist = None

    def fold(begin, end, logits):
        nonlocal hist
        logits = metric._device_result(logits, 'classify_fn', torch.float32)
        if hist is None:
            hist = hip_ops.ClassHistogram(logits.shape[1], logits.device)
        hist.update(logits)

    metric._walk(Gs, Gs_kwargs, 'fake', metric.classify_fn, fold, 'images', shard=(rank, world), as_uint8=False)
    return hist


def merged_class_counts(metric, Gs, Gs_kwargs):
    """Under metric._process_group: this rank's shard folded, then the total over all ranks (the same integers on every rank)."""
    import torch
    from .. import hip_ops
    group = metric._process_group
    rank, world = torch.distributed.get_rank(group), torch.distributed.get_world_size(group)
    hist = shard_histogram(metric, Gs, Gs_kwargs, rank, world)
    K = metric._agree_on_width(hist.K if hist is not None else 0, Gs.device, 'logit')
    if hist is None:
        hist = hip_ops.ClassHistogram(K, Gs.device)
    return hist.all_merge(group).to_host()


class mode_counts(metric_base.MetricBase):
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
                self._report_result(count_modes_from_counts(counts))
            return
        counts, labels_all, _ = class_statistics(self, Gs, Gs_kwargs, num_gpus)
        self._report_result(count_modes_from_counts(counts) if counts is not None else count_modes(labels_all))
