"""Train the Stacked-MNIST mode classifier (training/networks_classifier.py) that mode_counts_24k / KL24k read from
metrics/stacked_mnist_classifier.pkl -- the reference ships the metrics (metrics/mode_counts.py:29) but neither that file
nor its trainer, so this project trains its own:

    python -m inclusivegan_amd.train_classifier --data-dir D --dataset stacked_mnist_240k --out metrics/stacked_mnist_classifier.pkl

The one-hot labels `dataset_tool.py create_mnistrgb` writes are the supervision; in `digits` mode every colour plane is a
sample of one 10-way digit classifier (label digit = (number // place value) % 10), in `onehot` mode the whole image is a
sample of a K-way classifier.  The loss is hip_ops.SoftmaxXentFn (csrc/softmax_xent.hip), the update tflib.Optimizer (the Adam
kernel behind the finite check); a tick's mean loss and accuracy come from hip_ops.XentStats, one device
-> host copy per tick.  Eager, one process, one seeded RandomState; no hipGraph capture and no process group.

The classifier is this project's own: mode counts are comparable between models evaluated with the same pickle, not with
numbers obtained with the reference's unpublished one.

`--mode attributes` trains the CelebA attribute classifier that `ls` (metrics/linear_separability.py) reads from
metrics/celeba_attribute_classifier.pkl -- the reference downloads 40 CelebA-HQ classifiers from URLs this tree never opens:

    python -m inclusivegan_amd.train_classifier --mode attributes --data-dir D --dataset celeba_align_png_cropped_30k

The 40 binary attributes `dataset_tool.py create_celeba` writes (float32 {0, 1}, the columns of imle.CELEBA_ATTRIBUTES) are the
targets as they stand; the network is C_digits(per_channel=False, num_classes=A), one forward for all attributes; the loss is
hip_ops.SigmoidXentFn (csrc/sigmoid_xent.hip), optionally with pos_weight = negatives / positives per attribute; a tick's
per-attribute mean loss, accuracy and balanced accuracy come from hip_ops.BinaryXentStats.  This too is the project's own
network: `ls` numbers obtained with it are comparable between models evaluated with the same pickle, not with numbers obtained
with the reference's CelebA-HQ classifiers.  The defaults of --kimg and --lrate are untested on real CelebA."""
import argparse
import os
import sys
import time

import numpy as np
import torch

from . import hip_ops
from .dnnlib import tflib
from .dnnlib.tflib.network import network_from_state
from .training import dataset as dataset_mod, misc
from .training import networks_classifier as NC

DEFAULT_PKL = 'metrics/stacked_mnist_classifier.pkl'      # the reference's path, relative to the working directory
DEFAULT_ATTRIBUTE_PKL = 'metrics/celeba_attribute_classifier.pkl'      # where metrics/linear_separability.py looks
MODES = ('digits', 'onehot', 'attributes')
C_FUNC = 'inclusivegan_amd.training.networks_classifier.C_digits'


def class_targets(onehot, mode):
    """one-hot labels [n, K] float -> int32 targets: [n] class indices (onehot) or [3 n] digits, row n * 3 + c (digits)."""
    numbers = np.argmax(np.asarray(onehot), axis=1)
    if mode == 'onehot':
        return numbers.astype(np.int32)
    return NC.digits_of_number(numbers).reshape(-1).astype(np.int32)


def logit_rows(net, images, labels_stub):
    """The network's logits as the [rows, K] matrix the loss takes: [3 n, 10] in digit mode, [n, K] otherwise."""
    out = net.get_output_for(images, labels_stub, is_training=True)
    return out.reshape(-1, out.shape[-1])


def balanced_pos_weight(labels):
    """w_a = negatives / positives of every column of labels [n, A] in {0, 1} (float32 array); an attribute that lacks either raises."""
    labels = np.asarray(labels)
    pos, neg = np.sum(labels == 1, axis=0), np.sum(labels == 0, axis=0)
    bad = np.flatnonzero((pos == 0) | (neg == 0))
    if bad.size:
        raise ValueError('train_classifier: --pos-weight balanced needs a positive and a negative of every attribute in the training part; '
                         'attribute %d has %d positives and %d negatives' % (bad[0], pos[bad[0]], neg[bad[0]]))
    return (neg.astype(np.float64) / pos.astype(np.float64)).astype(np.float32)


def evaluate_attributes(net, images_u8, targets, minibatch):
    """(errors, pairs) of the network on uint8 device images against float32 device targets [n, A]: the (image, attribute)
    pairs whose target is 0 or 1, wrong where logit > 0 disagrees with it."""
    stats = hip_ops.BinaryXentStats(int(targets.shape[1]), images_u8.device)
    stub = torch.zeros(minibatch, 0, device=images_u8.device)
    with torch.no_grad():
        for b in range(0, images_u8.shape[0], minibatch):
            x = tflib.convert_images_from_uint8(images_u8[b:b + minibatch], drange=[-1, 1])
            t = targets[b:b + minibatch]
            logits = logit_rows(net, x, stub[:x.shape[0]]).contiguous()
            loss, _ = hip_ops.sigmoid_xent_raw(logits, t, return_pred=False)
            stats.update(loss, logits, t)
    _, counts = stats.sums()
    return int(counts[:, 1].sum() + counts[:, 3].sum()), int(counts.sum())


def evaluate(net, images_u8, targets, minibatch):
    """(errors, rows) of the network on uint8 device images against int32 device targets: arg-max of the loss kernel; float32
    targets [n, A] (attributes mode) go to evaluate_attributes."""
    if targets.dtype == torch.float32:
        return evaluate_attributes(net, images_u8, targets, minibatch)
    rows_per_image = targets.shape[0] // images_u8.shape[0]
    stats = hip_ops.XentStats(int(net.static_kwargs.get('num_classes', 10)), images_u8.device)
    stub = torch.zeros(minibatch, 0, device=images_u8.device)
    with torch.no_grad():
        for b in range(0, images_u8.shape[0], minibatch):
            x = tflib.convert_images_from_uint8(images_u8[b:b + minibatch], drange=[-1, 1])
            t = targets[b * rows_per_image:(b + minibatch) * rows_per_image]
            loss, _, pred = hip_ops.softmax_xent_raw(logit_rows(net, x, stub[:x.shape[0]]).contiguous(), t)
            stats.update(loss, t, pred)
    _, counted, correct = stats.sums()
    return counted - correct, counted


def train_classifier(images, onehot, out=None, mode='digits', kimg=600.0, minibatch=256, lrate=0.002, holdout=10000, seed=0,
                     fmap_base=1 << 10, tick_kimg=20.0, device=None, net=None, total_steps=None, log=print, pos_weight='none'):
    """Train on uint8 images [N, C, H, W] with one-hot labels [N, K] (NumPy), keeping the last `holdout` images out of training.
    Batches are drawn from one RandomState(seed) over the training part.  `net`: start from this Network (tests); `total_steps`
    overrides `kimg`.  Returns (network, record) with record = dict(steps, holdout_errors, holdout_rows, sec_per_step, ticks);
    writes the network to `out` in the Network pickle layout when given.

    mode 'attributes': `onehot` holds binary attributes [N, A] in {0, 1} instead, every (image, attribute) pair is a row of the
    record, and pos_weight 'balanced' weighs attribute a's positives by negatives / positives over the training part."""
    if mode not in MODES or pos_weight not in ('none', 'balanced'):
        raise ValueError('train_classifier: mode is one of %s and pos_weight none or balanced (got %r, %r)' % (MODES, mode, pos_weight))
    attrs = mode == 'attributes'
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    images = np.asarray(images)
    n_all, channels, res = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    holdout = int(holdout)
    if not 0 <= holdout < n_all:
        raise ValueError('train_classifier: holdout must leave at least one training image (%d of %d)' % (holdout, n_all))
    n_train = n_all - holdout
    K = int(np.asarray(onehot).shape[1])
    if mode == 'digits' and (K != 1000 or channels != 3):
        raise ValueError('train_classifier: digits mode takes three-channel images with 1000-way one-hot labels (got %d channels, %d classes)' % (channels, K))
    num_classes = 10 if mode == 'digits' else K
    rows_per_image = 3 if mode == 'digits' else 1
    if net is None:
        net = tflib.Network('C', func_name=C_FUNC, num_channels=channels, resolution=res, num_classes=num_classes,
                            per_channel=(mode == 'digits'), fmap_base=fmap_base, architecture='resnet', device=device, seed=seed)
    dev_images = torch.from_numpy(np.ascontiguousarray(images)).to(device)
    if attrs:                                                   # the labels as they stand: float32 [N, A], row = image
        host_targets = np.ascontiguousarray(np.asarray(onehot, dtype=np.float32))
        dev_targets = torch.from_numpy(host_targets).to(device)
        weights = torch.from_numpy(balanced_pos_weight(host_targets[:n_train])).to(device) if pos_weight == 'balanced' else None
    else:
        dev_targets = torch.from_numpy(class_targets(onehot, mode)).to(device)
    opt =tflib.Optimizer(name='TrainC', learning_rate=float(lrate), beta1=0.9, beta2=0.999, epsilon=1e-8)
    rng = np.random.RandomState(seed)
    steps = int(total_steps) if total_steps is not None else max(1, int(np.ceil(kimg * 1000 / minibatch)))
    tick_steps = max(1, int(round(tick_kimg * 1000 / minibatch)))
    stats = hip_ops.BinaryXentStats(num_classes, device) if attrs else hip_ops.XentStats(num_classes, device)
    stub = torch.zeros(minibatch, 0, device=device)
    row_offsets = torch.arange(rows_per_image, device=device)
    ticks, step_times = [], []
    t_tick = time.time()
    for step in range(1, steps + 1):
        idx = torch.from_numpy(rng.randint(n_train, size=minibatch)).to(device)
        x = tflib.convert_images_from_uint8(dev_images[idx], drange=[-1, 1])
        t = dev_targets[(idx[:, None] * rows_per_image + row_offsets[None, :]).reshape(-1)]
        if attrs:
            logits = logit_rows(net, x, stub)
            loss, _ = hip_ops.SigmoidXentFn.apply(logits, t, weights)
        else:
            loss, pred = hip_ops.SoftmaxXentFn.apply(logit_rows(net, x, stub), t)
        opt.register_gradients(loss.mean(), net)
        opt.apply_updates()
        if attrs:
            stats.update(loss, logits, t)
        else:
            stats.update(loss, t, pred)
        if step % tick_steps == 0 or step == steps:
            if attrs:                                             # the tick's one device -> host copy (it also ends the tick's clock)
                loss_sums, counts = stats.sums()
                _, _, balanced = stats.rates(loss_sums, counts)
                pairs = max(int(counts.sum()), 1)
                mean_loss, acc = float(loss_sums.sum() / pairs), float((counts[:, 0] + counts[:, 2]).sum() / pairs)
                worst = int(np.nanargmin(balanced)) if np.isfinite(balanced).any() else 0
            else:
                mean_loss, acc = stats.to_host()
            done = tick_steps if step % tick_steps == 0 else step % tick_steps
            step_times.append((time.time() - t_tick) / done)
            stats.reset()
            errs, rows = evaluate(net, dev_images[n_train:], dev_targets[n_train * rows_per_image:], minibatch) if holdout else (0, 0)
            held = 1.0 - errs / rows if rows else float('nan')
            ticks.append(dict(step=step, kimg=step * minibatch / 1000.0, loss=mean_loss, accuracy=acc, holdout_accuracy=held))
            if attrs:
                ticks[-1].update(worst_attribute=worst, worst_balanced_accuracy=float(balanced[worst]))
                log('tick %-4d kimg %-8.1f loss %-10.6f accuracy %-8.4f worst balanced accuracy %-8.4f (attribute %d) holdout accuracy %-8.4f sec/step %.5f'
                    % (len(ticks), step * minibatch / 1000.0, mean_loss, acc, balanced[worst], worst, held, step_times[-1]))
            else:
                log('tick %-4d kimg %-8.1f loss %-10.6f accuracy %-8.4f holdout accuracy %-8.4f sec/step %.5f'
                    % (len(ticks), step * minibatch / 1000.0, mean_loss, acc, held, step_times[-1]))
            t_tick = time.time()
    errs, rows = evaluate(net, dev_images[n_train:], dev_targets[n_train * rows_per_image:], minibatch) if holdout else (0, 0)
    if opt.overflow_count():
        log('%d steps were skipped for non-finite gradients' % opt.overflow_count())
    if out is not None:
        if os.path.dirname(out):
            os.makedirs(os.path.dirname(out), exist_ok=True)
        misc.save_pkl(net, out)
    return net, dict(steps=steps, holdout_errors=int(errs), holdout_rows=int(rows), ticks=ticks,
                     sec_per_step=float(np.median(step_times)) if step_times else float('nan'))


def load_classify_fn(pkl=DEFAULT_PKL, device=None):
    """The classifier of a pickle train_classifier wrote, as the metrics' `classify_fn`: float images [n, C, H, W] in [-1, 1]
    -> float32 device logits [n, K]; a per-channel digit classifier answers through networks_classifier.joint_logits
    ([n, 1000] joint log-probabilities)."""
    net, device = _load_network(pkl, device)
    per_channel = bool(net.static_kwargs.get('per_channel', True))

    def classify_fn(images):
        with torch.no_grad():
            images = torch.as_tensor(images).to(device=device, dtype=torch.float32)
            out = net.get_output_for(images, torch.zeros(images.shape[0], 0, device=device), is_training=False)
            return (NC.joint_logits(out) if per_channel else out).contiguous()

    classify_fn.network = net
    return classify_fn


class AttributeClassifier:
    """The attribute classifier of a pickle train_classifier wrote in `attributes` mode, in the shape `ls` takes:
    classify_all(images) is ONE forward for all attributes, float images [n, C, H, W] in G's range -> float32 device logits
    [n, A] in the columns the network was trained on (imle.CELEBA_ATTRIBUTES for a CelebA set); `idx in c` and `c[idx]` speak
    linear separability's attribute index (linear_separability.LS_ATTRIBUTE_NAMES), c[idx] being a callable(images) -> logits
    [n, 1], so that the object can be injected as `classify_fns` as it stands.  Images at an integer multiple of the classifier's
    resolution are box-mean downsampled (the reference does the same for its 256 x 256 classifiers, :128-131); any other size
    raises."""

    def __init__(self, network, device):
        self.network, self.device = network, device
        self.num_attributes = int(network.static_kwargs['num_classes'])
        self.resolution = int(network.static_kwargs['resolution'])

    def classify_all(self, images):
        with torch.no_grad():
            images = torch.as_tensor(images).to(device=self.device, dtype=torch.float32)
            res = self.resolution
            if images.dim() != 4 or images.shape[2] != images.shape[3] or images.shape[2] < res or images.shape[2] % res:
                raise ValueError('attribute classifier: images must be [n, C, H, H] with H a multiple of %d (got %s)' % (res, tuple(images.shape)))
            factor = images.shape[2] // res
            if factor > 1:
                images = images.reshape(-1, images.shape[1], res, factor, res, factor).mean(dim=(3, 5))
            return self.network.get_output_for(images, torch.zeros(images.shape[0], 0, device=self.device), is_training=False).contiguous()

    def __contains__(self, attrib_idx):
        from .metrics.linear_separability import LS_ATTRIBUTE_NAMES, attribute_column
        return isinstance(attrib_idx, (int, np.integer)) and 0 <= attrib_idx < len(LS_ATTRIBUTE_NAMES) and attribute_column(attrib_idx) < self.num_attributes

    def __getitem__(self, attrib_idx):
        from .metrics.linear_separability import attribute_column
        if attrib_idx not in self:
            raise KeyError(attrib_idx)
        column = attribute_column(attrib_idx)
        return lambda images: self.classify_all(images)[:, column:column + 1]


def _load_network(pkl, device):
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    net = misc.as_networks(misc.load_pkl(pkl), device=device)
    if net.device != device:        # a plain pickle comes back on the device it was written from
        net = network_from_state(net.state_v4(), device=device)
    return net, device


def load_attribute_classifier(pkl=DEFAULT_ATTRIBUTE_PKL, device=None):
    """The AttributeClassifier of a pickle train_classifier wrote in `attributes` mode."""
    net, device = _load_network(pkl, device)
    if net.static_kwargs.get('per_channel', True):
        raise ValueError('load_attribute_classifier: %s holds a per-channel digit classifier, not an attribute classifier' % pkl)
    return AttributeClassifier(net, device)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Train the Stacked-MNIST mode classifier that mode_counts_24k / KL24k read, or (--mode attributes) '
                                            'the CelebA attribute classifier that ls reads.',
                                epilog='The defaults of --kimg and --lrate are untested against real digits and against real CelebA in this '
                                       'tree: check the held-out accuracy the run prints before trusting a mode count or an ls value.')
    p.add_argument('--data-dir', required=True, help='Dataset root directory')
    p.add_argument('--dataset', required=True, help='TFRecord directory under --data-dir (e.g. stacked_mnist_240k)')
    p.add_argument('--out', default=None, help='Pickle to write (default: %s; in attributes mode %s)' % (DEFAULT_PKL, DEFAULT_ATTRIBUTE_PKL))
    p.add_argument('--kimg', type=float, default=600.0, help='Thousands of images to train on (default: %(default)s; not tuned on real digits or real CelebA)')
    p.add_argument('--minibatch', type=int, default=256, help='Images per step (default: %(default)s)')
    p.add_argument('--lrate', type=float, default=0.002, help='Adam learning rate (default: %(default)s; not tuned on real digits or real CelebA)')
    p.add_argument('--holdout', type=int, default=10000, help='Last images of the set kept out of training (default: %(default)s)')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--fmap-base', type=int, default=1 << 10, help='Width of the network: feature maps at stage s = fmap_base / 2^s (default: %(default)s)')
    p.add_argument('--mode', choices=list(MODES), default='digits',
                   help='digits: one 10-way classifier applied to each colour plane (Stacked MNIST); onehot: K-way on the whole image; '
                        'attributes: one sigmoid output per binary attribute column (CelebA)')
    p.add_argument('--pos-weight', choices=['none', 'balanced'], default='none',
                   help='attributes mode: balanced weighs the positives of attribute a by negatives / positives over the training part (default: %(default)s)')
    a = p.parse_args(argv)
    if a.out is None:
        a.out = DEFAULT_ATTRIBUTE_PKL if a.mode == 'attributes' else DEFAULT_PKL
    if a.pos_weight != 'none' and a.mode != 'attributes':
        p.error('--pos-weight applies to --mode attributes')
    return a


def main(argv=None):
    a = parse_args(argv)
    ds = dataset_mod.load_dataset(data_dir=a.data_dir, tfrecord_dir=a.dataset, max_label_size='full')
    if ds.label_size < 2:
        sys.exit('train_classifier: %s has no one-hot labels' % os.path.join(a.data_dir, a.dataset))
    _, rec = train_classifier(ds._images, ds._labels, out=a.out, mode=a.mode, kimg=a.kimg, minibatch=a.minibatch, lrate=a.lrate,
                              holdout=min(a.holdout, ds.data_size - 1), seed=a.seed, fmap_base=a.fmap_base, pos_weight=a.pos_weight)
    print('wrote %s: %d steps, %.5f s/step, held-out errors %d of %d' % (a.out, rec['steps'], rec['sec_per_step'], rec['holdout_errors'], rec['holdout_rows']))


if __name__ == '__main__':
    main()
