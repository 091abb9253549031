"""GPU: the CelebA attribute classifier (train_classifier.py --mode attributes, the sigmoid cross-entropy of
csrc/sigmoid_xent.hip) against the fp64 restatement of tests/test_gpu_classifier.py: forward, mean loss and the gradient of
every trainable at 32 x 32 with five attributes, a learning run on a synthetic glyph set next to the same run in fp64 on the
CPU, the pickle round trip, and linear separability's pick-up of the written pickle.

Thresholds are those tests/test_gpu_classifier.py states: outputs 1e-4, the loss value 2e-4, gradients 5e-3 in relative L2 per
tensor.

The learning run (chosen on the CPU, by the fp64 run alone): five fixed seeded glyphs -- patterns of 4 x 4 blocks over the three
colour planes of a 32 x 32 image, a fifth of the blocks set -- each present or absent independently, glyph 3 with probability
1/8 and the others with 1/2; an image is 48 + 40 x (the sum of its glyphs) plus Gaussian noise of sigma NOISE = 6 on the
0..255 scale.  LEARN_IMAGES = 320 images of which the last LEARN_HOLDOUT = 64 are held out (320 pairs); LEARN_STEPS = 80 steps of
LEARN_MB = 16 images at LEARN_LRATE = 0.01.  The fp64 run classifies all 320 held-out pairs correctly with a smallest |logit| of
2.87 and a loss falling from 0.728 to 0.0034 (60 steps: 41 errors; sigma 8 with 80 steps: 1 error, smallest |logit| 0.57, both
rejected; sigma 8 with 100 steps: 0 errors, 2.93, but a longer test); the HIP run may make at most 1 % of the pairs more errors."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.util import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A = 5
RARE = 3                     # the glyph present with probability 1/8
NOISE, LEARN_IMAGES, LEARN_HOLDOUT, LEARN_STEPS, LEARN_MB, LEARN_LRATE = 6.0, 320, 64, 80, 16, 0.01
LS_ATTRIBS = [5, 6, 2, 7, 8]      # linear separability's indices of the data set's columns 0..4 (5_o_Clock_Shadow .. Bald)


def attribute_set(num_images, noise, seed=0):
    """uint8 images [n, 3, 32, 32] of noisy glyph sums and their float32 {0, 1} attribute labels [n, 5] (create_celeba's layout)."""
    from tests.test_gpu_classifier import RES
    rng = np.random.RandomState(seed)
    glyphs = np.kron((rng.rand(A, 3, 8, 8) < 0.2).astype(np.float64), np.ones((4, 4)))        # 4x4 blocks: they survive the FIR downsampling
    prob = np.full(A, 0.5)
    prob[RARE] = 0.125
    present = rng.rand(num_images, A) < prob[None, :]
    clean = 48.0 + 40.0 * np.einsum('na,achw->nchw', present.astype(np.float64), glyphs)
    images = np.clip(np.rint(clean + noise * rng.randn(num_images, 3, RES, RES)), 0, 255).astype(np.uint8)
    return images, present.astype(np.float32)


def test_forward_loss_and_gradients_match_fp64(cuda_device):
    from inclusivegan_amd import hip_ops
    from tests.test_gpu_classifier import RES, c_digits_oracle, grad_errs, make_net, oracle_params
    dev = cuda_device
    net = make_net(dev, False, A)
    assert tuple(net.vars['Output/weight'].shape)[1] == A and net.static_kwargs['per_channel'] is False
    N = 6
    g = torch.Generator().manual_seed(3)
    img = (torch.rand(N, 3, RES, RES, generator=g) * 2 - 1).to(dev)
    stub = torch.zeros(N, 0, device=dev)
    targets = (torch.rand(N, A, generator=g) < 0.5).to(torch.float32)
    targets[2, 1] = -1.0                                               # a padding element: no loss, no gradient
    w = torch.tensor([1.0, 0.5, 3.0, 7.0, 1.5])
    with torch.no_grad():
        out = net.get_output_for(img, stub, is_training=False)
    assert tuple(out.shape) == (N, A)
    op = oracle_params(net)
    out_o = c_digits_oracle(op, img.double().cpu(), A, False)
    print('forward rel err %.3e' % rel_err(out, out_o))
    assert rel_err(out, out_o) < 1e-4
    for weight in (None, w):
        net.zero_grad()
        for p in op.values():
            p.grad = None
        logits = net.get_output_for(img, stub, is_training=True)
        loss, pred = hip_ops.SigmoidXentFn.apply(logits, targets.to(dev), None if weight is None else weight.to(dev))
        torch.autograd.backward(loss.mean(), inputs=list(net.trainables.values()))
        out_o = c_digits_oracle(op, img.double().cpu(), A, False)
        counted = (targets >= 0).double()
        per = torch.nn.functional.binary_cross_entropy_with_logits(out_o, targets.double().clamp(min=0), reduction='none',
                                                                   pos_weight=None if weight is None else weight.double())
        loss_o = (per * counted).sum() / (N * A)                       # the trainer's mean runs over all elements, the padding's 0 included
        loss_o.backward()
        print('loss %.6f (oracle %.6f)' % (float(loss.detach().mean()), float(loss_o.detach())))
        assert rel_err(loss.mean(), loss_o) < 2e-4 and float(loss[2, 1]) == 0.0
        assert np.array_equal(pred.cpu().numpy(), (logits.detach().cpu().numpy() > 0).astype(np.int8))
        errs = grad_errs(net, op)
        worst = max(errs, key=errs.get)
        print('worst gradient: %s %.3e' % (worst, errs[worst]))
        assert errs[worst] < 5e-3, (worst, errs[worst])


# ---- the learning run ----------------------------------------------------------------------------------------------------------
def oracle_training_run(params, images_u8, targets, n_train, steps, minibatch, lrate, seed):
    """train_classifier's attributes loop in fp64 on the CPU: the same draws, the mean loss over all pairs, Adam as
    tflib.Optimizer states it.  -> (held-out errors, held-out pairs, smallest |logit| on the held-out pairs, first and last loss)."""
    from tests.test_gpu_classifier import c_digits_oracle
    names = [n for n, p in params.items() if p.requires_grad]
    m = {n: torch.zeros_like(params[n]) for n in names}
    v = {n: torch.zeros_like(params[n]) for n in names}
    b1, b2, eps = 0.9, 0.999, 1e-8
    x_all = torch.from_numpy(images_u8.astype(np.float64)) * (2.0 / 255.0) - 1.0
    t_all = torch.from_numpy(targets.astype(np.float64))
    rng = np.random.RandomState(seed)
    losses = []
    for step in range(1, steps + 1):
        idx = torch.from_numpy(rng.randint(n_train, size=minibatch))
        logits = c_digits_oracle(params, x_all[idx], targets.shape[1], False)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, t_all[idx])
        losses.append(float(loss.detach()))
        grads = torch.autograd.grad(loss, [params[n] for n in names])
        lr_t = lrate * np.sqrt(1 - b2 ** step) / (1 - b1 ** step)
        with torch.no_grad():
            for n, g in zip(names, grads):
                m[n].mul_(b1).add_(g, alpha=1 - b1)
                v[n].mul_(b2).addcmul_(g, g, value=1 - b2)
                params[n].sub_(lr_t * m[n] / (v[n].sqrt() + eps))
    with torch.no_grad():
        logits = c_digits_oracle(params, x_all[n_train:], targets.shape[1], False)
    errors = int(((logits > 0).double() != t_all[n_train:]).sum())
    return errors, int(logits.numel()), float(logits.abs().min()), losses[0], losses[-1]


@pytest.fixture(scope='module')
def learning_run(cuda_device, tmp_path_factory):
    """One training run shared by the tests below: the set written as TFRecords and read back, the HIP run through
    train_classifier's function entry point, the fp64 run from the same initial weights."""
    from inclusivegan_amd import train_classifier as TC
    from inclusivegan_amd.training import dataset as dataset_mod
    from inclusivegan_amd.training.tfrecord import TFRecordExporter
    from tests.test_gpu_classifier import make_net, oracle_params
    root = tmp_path_factory.mktemp('attributes')
    images, labels = attribute_set(LEARN_IMAGES, NOISE)
    with TFRecordExporter(str(root / 'glyph_attributes'), LEARN_IMAGES, print_progress=False) as tfr:
        for img in images:
            tfr.add_image(img)
        tfr.add_labels(labels)
    ds = dataset_mod.load_dataset(data_dir=str(root), tfrecord_dir='glyph_attributes', max_label_size='full')
    assert np.array_equal(ds._images, images) and np.array_equal(ds._labels, labels) and ds._labels.dtype == np.float32
    net = make_net(cuda_device, False, A, seed=33, bias_noise=False)
    op = oracle_params(net)
    pkl = str(root / 'metrics' / 'celeba_attribute_classifier.pkl')
    lines = []
    net, rec = TC.train_classifier(ds._images, ds._labels, out=pkl, mode='attributes', minibatch=LEARN_MB, lrate=LEARN_LRATE,
                                   holdout=LEARN_HOLDOUT, seed=5, net=net, total_steps=LEARN_STEPS, tick_kimg=LEARN_MB * 20 / 1000.0,
                                   device=cuda_device, log=lambda s: (print(s), lines.append(s)))
    oracle = oracle_training_run(op, images, labels, LEARN_IMAGES - LEARN_HOLDOUT, LEARN_STEPS, LEARN_MB, LEARN_LRATE, seed=5)
    return dict(root=root, pkl=pkl, images=images, labels=labels, net=net, rec=rec, oracle=oracle, lines=lines)


def test_learning_run_next_to_the_fp64_run(learning_run):
    rec = learning_run['rec']
    o_err, o_pairs, o_min, o_first, o_last = learning_run['oracle']
    print('fp64 run: %d errors of %d held-out pairs, smallest |logit| %.4f, loss %.4f -> %.4f; HIP run: %d errors of %d; %.5f s/step'
          % (o_err, o_pairs, o_min, o_first, o_last, rec['holdout_errors'], rec['holdout_rows'], rec['sec_per_step']))
    assert o_err == 0 and o_pairs == A * LEARN_HOLDOUT, 'the condition of this test: the fp64 run alone classifies every held-out pair'
    assert rec['holdout_rows'] == o_pairs and rec['steps'] == LEARN_STEPS
    assert rec['holdout_errors'] <= o_err + 0.01 * o_pairs
    assert len(rec['ticks']) == 4 and all(np.isfinite(t['loss']) and 0 <= t['accuracy'] <= 1 for t in rec['ticks'])
    assert rec['ticks'][-1]['loss'] < rec['ticks'][0]['loss']
    assert all(0 <= t['worst_attribute'] < A and 0 <= t['worst_balanced_accuracy'] <= 1 for t in rec['ticks'])
    assert all('worst balanced accuracy' in line and '(attribute %d)' % t['worst_attribute'] in line for line, t in zip(learning_run['lines'], rec['ticks']))


def test_balanced_pos_weight_trains_and_an_empty_class_raises(learning_run, cuda_device):
    from inclusivegan_amd import train_classifier as TC
    from tests.test_gpu_classifier import make_net
    images, labels = learning_run['images'][:32], learning_run['labels'][:32]
    net = make_net(cuda_device, False, A, seed=33, bias_noise=False)
    _, rec = TC.train_classifier(images, labels, mode='attributes', minibatch=8, lrate=LEARN_LRATE, holdout=8, seed=5, net=net, total_steps=3,
                                 device=cuda_device, log=lambda s: None, pos_weight='balanced')
    assert np.isfinite(rec['ticks'][-1]['loss']) and rec['holdout_rows'] == 8 * A
    one_class = labels.copy()
    one_class[:, 2] = 0.0
    with pytest.raises(ValueError, match='attribute 2 has 0 positives'):
        TC.train_classifier(images, one_class, mode='attributes', minibatch=8, holdout=8, net=net, total_steps=1, device=cuda_device,
                            log=lambda s: None, pos_weight='balanced')


def test_pickle_round_trip_reproduces_the_trainers_count(learning_run, cuda_device):
    from inclusivegan_amd import train_classifier as TC
    from inclusivegan_amd.dnnlib import tflib
    from inclusivegan_amd.metrics.linear_separability import attribute_column
    c = TC.load_attribute_classifier(learning_run['pkl'], device=cuda_device)
    assert c.network is not learning_run['net'] and c.network.static_kwargs['per_channel'] is False and c.num_attributes == A
    held = tflib.convert_images_from_uint8(torch.from_numpy(learning_run['images'][-LEARN_HOLDOUT:]).to(cuda_device), drange=[-1, 1])
    logits = c.classify_all(held)
    assert logits.dtype == torch.float32 and logits.is_cuda and tuple(logits.shape) == (LEARN_HOLDOUT, A)
    wrong = (logits.cpu().numpy() > 0) != (learning_run['labels'][-LEARN_HOLDOUT:] == 1.0)
    assert int(wrong.sum()) == learning_run['rec']['holdout_errors']    # pair by pair, the trainer's own count
    # the per-attribute view linear separability's torch path takes, in the reference's numbering
    assert [a in c for a in LS_ATTRIBS] == [True] * A and 0 not in c and 39 not in c and 40 not in c and 'x' not in c
    for a in LS_ATTRIBS:
        one = c[a](held)
        assert tuple(one.shape) == (LEARN_HOLDOUT, 1) and torch.equal(one[:, 0], logits[:, attribute_column(a)])
    with pytest.raises(KeyError):
        c[0]
    # an integer multiple of the resolution is box-mean downsampled; anything else raises
    doubled = held.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    assert torch.equal(c.classify_all(doubled), logits)
    for bad in (held[:, :, :24, :24], torch.nn.functional.pad(held, (0, 16, 0, 16)), held[:, :, :, :16]):
        with pytest.raises(ValueError, match='multiple of 32'):
            c.classify_all(bad)
    from inclusivegan_amd.training import misc
    from tests.test_gpu_classifier import make_net
    digits = str(learning_run['root'] / 'digits.pkl')
    misc.save_pkl(make_net(cuda_device, True, 10), digits)
    with pytest.raises(ValueError, match='per-channel digit classifier'):
        TC.load_attribute_classifier(digits, device=cuda_device)


def test_ls_picks_the_pickle_up(learning_run, cuda_device, monkeypatch):
    """classify_fns=None with the pickle at classifier_pkl reports exactly what injecting load_attribute_classifier(pkl) reports;
    against the same network injected as plain per-attribute callables (the torch path) the targets agree on every sample whose
    logit is not 0 and the probabilities agree within one fp32 spacing at 1 (2^-23, the scale of a probability pair: the torch
    path rounds exp, 1 + e and the quotient in fp32, up to 1.5 spacings of [0.5, 1) for the larger probability and far less for
    the smaller, the HIP path rounds once)."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import class_dist_worker as W
    from inclusivegan_amd import train_classifier as TC
    from inclusivegan_amd.metrics import linear_separability as ls
    was = torch.is_grad_enabled()
    try:
        Gs = W.make_gs(cuda_device)
        pkl = learning_run['pkl']
        c = TC.load_attribute_classifier(pkl, device=cuda_device)
        forwards, logits_seen = [], {a: [] for a in LS_ATTRIBS}
        classify_all = c.classify_all
        c.classify_all = lambda images: (forwards.append(int(images.shape[0])), classify_all(images))[1]

        def plain(a):
            def fn(images):
                out = classify_all(images)[:, ls.attribute_column(a):ls.attribute_column(a) + 1]
                logits_seen[a].append(out)
                return out
            return fn

        base = dict(num_samples=96, num_keep=48, attrib_indices=LS_ATTRIBS, minibatch_per_gpu=8, name='ls_tiny')
        runs = {}
        for key, kw in (('picked', dict(classifier_pkl=pkl)), ('injected', dict(classify_fns=c, classifier_pkl='/nonexistent.pkl')),
                        ('plain', dict(classify_fns={a: plain(a) for a in LS_ATTRIBS}, classifier_pkl=pkl))):
            metric = ls.LS(**base, **kw)
            torch.manual_seed(77)
            metric.run(Gs, num_gpus=1)
            runs[key] = metric
        values = {key: [(r.suffix, r.value) for r in m._results] for key, m in runs.items()}
        print(values)
        assert values['picked'] == values['injected'] and [s for s, _ in values['picked']] == ['_z', '_w']
        assert all(np.isfinite(v) for _, v in values['picked'])
        assert forwards == [8] * 12                                        # one forward per minibatch, not one per attribute
        assert hasattr(runs['picked'].classify_fns, 'classify_all') and runs['plain'].classify_fns.keys() == set(LS_ATTRIBS)
        worst = 0.0
        for a in LS_ATTRIBS:
            hip, ref = runs['injected'].results[a], runs['plain'].results[a]
            assert torch.equal(runs['picked'].results[a], hip) and tuple(hip.shape) == (96, 2)
            x = torch.cat(logits_seen[a])[:96, 0]
            nonzero = x != 0
            assert torch.equal(ls.svm_targets_of(hip)[nonzero], ls.svm_targets_of(ref)[nonzero])
            clear = x.abs() > 2.0 ** -24                                   # below that both probabilities round to 0.5: a tie, target 0
            assert torch.equal(ls.svm_targets_of(hip)[clear], (x < 0).to(torch.int64)[clear])
            worst = max(worst, float((hip.double() - ref.double()).abs().max()))
        print('probabilities, HIP path against the torch path: worst difference %.3e (one fp32 spacing at 1 is %.3e)' % (worst, 2.0 ** -23))
        assert worst <= 2.0 ** -23
        # the reference's relative path, from the run's working directory
        monkeypatch.chdir(str(learning_run['root']))
        metric = ls.LS(**base)
        torch.manual_seed(77)
        metric.run(Gs, num_gpus=1)
        assert [(r.suffix, r.value) for r in metric._results] == values['picked']
        # a classifier without the attribute asked for is an error that says so
        with pytest.raises(RuntimeError, match='has 5 outputs and none for attribute indices \\[0\\]'):
            ls.LS(**dict(base, attrib_indices=[0, 5]))._evaluate(Gs, {}, 1)
    finally:
        torch.set_grad_enabled(was)
