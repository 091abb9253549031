"""Inception Score (reference: metrics/inception_score.py:18-56; Salimans et al., "Improved Techniques for Training GANs").

    per split: exp(mean over images of KL(p(y | x) || p(y))), p(y) the split's own mean; reported: mean and std over splits

The Inception-v3 softmax network of the reference (metrics/inception_v3_softmax.pkl) is not available; `IS` takes
`classify_fn(uint8 images [n, C, H, W] on the device) -> softmax probabilities [n, K]` instead, like `FID`'s `feature_fn`.
The statistic on top of it is host NumPy, value for value."""
import numpy as np
import torch

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
    def __init__(self, num_images, num_splits, minibatch_per_gpu, classify_fn=None, **kwargs):
        super().__init__(**kwargs)
        self.num_images = num_images
        self.num_splits = num_splits
        self.minibatch_per_gpu = minibatch_per_gpu
        self.classify_fn = classify_fn

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        if self.classify_fn is None:
            raise RuntimeError('IS needs classify_fn: the reference\'s metrics/inception_v3_softmax.pkl is not available in this tree')
        minibatch_size = num_gpus * self.minibatch_per_gpu
        activations = None

        # Calculate activations for fakes.
        for begin in range(0, self.num_images, minibatch_size):
            end = min(begin + minibatch_size, self.num_images)
            probs = torch.as_tensor(self.classify_fn(self._generate(Gs, minibatch_size, Gs_kwargs))).detach().to('cpu', torch.float32).numpy()
            if activations is None:
                activations = np.empty([self.num_images, probs.shape[1]], dtype=np.float32)
            activations[begin:end] = probs[:end - begin]

        # Calculate IS.
        scores = inception_score_splits(activations, self.num_splits)
        self._report_result(np.mean(scores), suffix='_mean')
        self._report_result(np.std(scores), suffix='_std')
