"""The Stacked-MNIST mode classifier: this project's own network, trained by this project's trainer (train_classifier.py).

The reference's metrics (metrics/mode_counts.py:29, metrics/KL.py) read metrics/stacked_mnist_classifier.pkl, a pre-trained
network whose trainer was never published.  `C_digits` stands in its place: the body of `D_stylegan2_feature`
(networks_stylegan2.py) on the same building blocks, WITHOUT the minibatch-stddev layer (a classifier's answer for one image
must not depend on the others of its batch) and with `num_classes` output units.

per_channel=True (Stacked MNIST): the three colour planes of an image are three independent digits (dataset_tool.py
create_mnistrgb: label = R digit + 10 G digit + 100 B digit), so they go through ONE single-channel digit classifier as three
rows -- [N, 3, H, W] -> [3N, 1, H, W] -> logits [N, 3, num_classes].  A digit classifier learnt once serves all three place
values and needs 10 classes' worth of data, not 1000.  `joint_logits` turns the three log-softmaxes into the [N, 1000] matrix
the metrics take.  per_channel=False: a plain `num_classes`-way classifier of the whole image, for any other one-hot-labelled
set.

Mode counts obtained with a classifier trained here are comparable between models evaluated with the same pickle; they are
not comparable to numbers obtained with the reference's unpublished pickle."""
import numpy as np
import torch

from .. import hip_ops
from ..dnnlib.tflib.tfutil import variable_scope
from ..dnnlib.tflib.ops.upfirdn_2d import downsample_2d
from .networks_stylegan2 import conv2d_layer, conv2d_bias_act_layer, dense_layer, apply_bias_act

PLACE_VALUES = (1, 10, 100)     # create_mnistrgb: number = R digit + 10 G digit + 100 B digit


def digits_of_number(numbers):
    """[...] integers 0..999 -> [..., 3] digits in channel order (R, G, B) = (ones, tens, hundreds)."""
    numbers = np.asarray(numbers, dtype=np.int64)
    return np.stack([(numbers // p) % 10 for p in PLACE_VALUES], axis=-1)


def number_of_digits(digits):
    """[..., 3] digits in channel order -> [...] numbers 0..999 (the inverse of digits_of_number)."""
    return np.asarray(digits, dtype=np.int64) @ np.asarray(PLACE_VALUES, dtype=np.int64)


def joint_logits(per_channel_logits):
    """[N, 3, 10] per-channel logits -> [N, 1000] float32 joint log-probabilities, the matrix `classify_fn` returns: entry
    r + 10 g + 100 b is log_softmax[0][r] + log_softmax[1][g] + log_softmax[2][b], summed in that order.

    Its arg-max is the triple of per-channel arg-maxes whenever each channel's top-two gap exceeds the fp32 rounding of the
    sum (a few 2^-24 of the summed magnitude).  Below that the sums of two different triples can round to the SAME float32,
    and np.argmax then reports the lower index: a lower-indexed near-tie collapses onto the maximum."""
    n, c, k = per_channel_logits.shape
    assert c == len(PLACE_VALUES) and k == 10
    # the 30 log-softmaxes of an image in fp64, each rounded to fp32 once: an fp32 log_softmax is wrong by an ulp of the
    # LOGIT's size, which for the winning class (log-probability near 0) is many ulps of the term itself
    ls = torch.log_softmax(per_channel_logits.to(torch.float64), dim=2).to(torch.float32)
    joint = (ls[:, 0, None, None, :] + ls[:, 1, None, :, None]) + ls[:, 2, :, None, None]      # [N, b, g, r]: index 100 b + 10 g + r
    return joint.reshape(n, k ** c)


def C_digits(
    images_in,
    labels_in,
    num_channels        = 3,
    resolution          = 32,
    label_size          = 0,            # width of labels_in (unused by the body, as in D)
    num_classes         = 10,
    per_channel         = True,         # classify every colour plane on its own with one single-channel network
    fmap_base           = 1 << 10,
    fmap_decay          = 1.0,
    fmap_min            = 1,
    fmap_max            = 512,
    architecture        = 'resnet',
    nonlinearity        = 'lrelu',
    dtype               = 'float32',
    resample_kernel     = [1,3,3,1],
    **_kwargs):

    resolution_log2 = int(np.log2(resolution))
    assert resolution == 2**resolution_log2 and resolution >= 4
    def nf(stage): return int(np.clip(int(fmap_base / (2.0 ** (stage * fmap_decay))), fmap_min, fmap_max))
    assert architecture in ['orig', 'skip', 'resnet']
    assert dtype == 'float32'
    act = nonlinearity
    assert tuple(images_in.shape[1:]) == (num_channels, resolution, resolution)
    images_in = images_in.to(torch.float32)
    num_images = int(images_in.shape[0])
    if per_channel:
        images_in = images_in.reshape(num_images * num_channels, 1, resolution, resolution)      # row n * C + c: plane c of image n
    if images_in.is_cuda:
        images_in = hip_ops.nhwc(images_in)

    def fromrgb(x, y, res):
        with variable_scope('FromRGB'):
            t = apply_bias_act(conv2d_layer(y, fmaps=nf(res-1), kernel=1), act=act)
            return t if x is None else x + t
    def block(x, res):
        t = x
        with variable_scope('Conv0'):
            x = conv2d_bias_act_layer(x, fmaps=nf(res-1), kernel=3, act=act)
        if architecture == 'resnet':        # (x + t) / sqrt(2) with the factor on the two branches' own multipliers, as in D
            from ..dnnlib.tflib.ops.fused_bias_act import activation_funcs
            c = 1 / np.sqrt(2)
            with variable_scope('Conv1_down'):
                x = conv2d_bias_act_layer(x, fmaps=nf(res-2), kernel=3, down=True, resample_kernel=resample_kernel, act=act,
                                          gain=float(activation_funcs[act].def_gain * c))
            with variable_scope('Skip'):
                t = conv2d_layer(t, fmaps=nf(res-2), kernel=1, down=True, resample_kernel=resample_kernel, gain=c)
                return x + t
        with variable_scope('Conv1_down'):
            return conv2d_bias_act_layer(x, fmaps=nf(res-2), kernel=3, down=True, resample_kernel=resample_kernel, act=act)

    x = None
    y = images_in
    for res in range(resolution_log2, 2, -1):
        with variable_scope('%dx%d' % (2**res, 2**res)):
            if architecture == 'skip' or res == resolution_log2:
                x = fromrgb(x, y, res)
            x = block(x, res)
            if architecture == 'skip':
                with variable_scope('Downsample'):
                    y = downsample_2d(y, k=resample_kernel)

    with variable_scope('4x4'):
        if architecture == 'skip':
            x = fromrgb(x, y, 2)
        with variable_scope('Conv'):
            x = conv2d_bias_act_layer(x, fmaps=nf(1), kernel=3, act=act)
        with variable_scope('Dense0'):
            x = apply_bias_act(dense_layer(x, fmaps=nf(0)), act=act)

    with variable_scope('Output'):
        x = apply_bias_act(dense_layer(x, fmaps=num_classes))
    if per_channel:
        x = x.reshape(num_images, num_channels, num_classes)
    return x
