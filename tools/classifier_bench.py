"""Measured record of the Stacked-MNIST mode classifier: the softmax cross-entropy kernel pair next to
torch.nn.functional.cross_entropy, the trainer's time per step, and the synthetic learning run of tests/test_gpu_classifier.py.

    python tools/classifier_bench.py [--calls 20000] [--windows 5] [--steps 60] [--mnist-dir DIR] [--out profiles/classifier.txt]

Part 1: forward + backward of hip_ops.SoftmaxXentFn (igan_softmax_xent_fwd / _bwd) at [768, 10] (3 x minibatch 256 digit rows)
and [256, 1000], and of F.cross_entropy(reduction='none') forward + backward on the same device tensors -- the path a user
would otherwise take; the parent tree has no such op, so there is no earlier time.  Stream time between two events around
`--calls` forward + backward pairs (a window of a second or more), the two sides alternating window by window after a warm-up
window of each, divided by the pairs: it contains whatever gap the host leaves between launches, for both sides alike.  The
kernels' own times come from `rocprofv3 --kernel-trace --stats -- python tools/classifier_bench.py --trace`, a run of its own.
Part 2: train_classifier's seconds per step at the default minibatch (256) and width on synthetic glyph images, eager.
Part 3: the learning run of tests/test_gpu_classifier.py (its parameters, the fp64 run's and the HIP run's held-out errors).
Part 4: with --mnist-dir holding the MNIST training files, the held-out accuracy after the default schedule; otherwise a line
saying it is unmeasured."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def xent_pairs(n, K, dev, gen):
    """The two sides on the same device tensors: forward + backward of hip_ops.SoftmaxXentFn and of F.cross_entropy."""
    import torch
    from inclusivegan_amd import hip_ops
    x = torch.randn(n, K, device=dev, generator=gen).requires_grad_(True)
    t32 = torch.randint(K, (n,), device=dev, generator=gen).to(torch.int32)
    t64 = t32.long()
    w = torch.full((n,), 1.0 / n, device=dev)

    def hip_pair():
        loss, _ = hip_ops.SoftmaxXentFn.apply(x, t32)
        torch.autograd.grad(loss, x, w)

    def torch_pair():
        loss = torch.nn.functional.cross_entropy(x, t64, reduction='none')
        torch.autograd.grad(loss, x, w)

    return hip_pair, torch_pair


def kernel_part(a, emit):
    import torch
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    names = ('hip_ops.SoftmaxXentFn (fp64 arithmetic, lse kept, arg-max included)', 'torch F.cross_entropy (fp32)')
    for n, K in ((768, 10), (256, 1000)):
        pairs = xent_pairs(n, K, dev, gen)
        for fn in pairs:                            # warm-up: both sides, a full window each
            for _ in range(a.calls):
                fn()
        torch.cuda.synchronize()
        per = ([], [])
        for _ in range(a.windows):                  # the sides alternate, window by window, in one process
            for side, fn in enumerate(pairs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                per[side].append(e0.elapsed_time(e1) / a.calls * 1e3)
        for side, name in enumerate(names):
            emit('[%d, %d] forward + backward, %s: median %.2f us per pair, min %.2f us, max %.2f us, of %d alternated windows of %d pairs (%.2f s each; launch gaps included)'
                 % (n, K, name, statistics.median(per[side]), min(per[side]), max(per[side]), a.windows, a.calls, statistics.median(per[side]) * a.calls * 1e-6))


def trace_part(a):
    """For `rocprofv3 --kernel-trace --stats -- python tools/classifier_bench.py --trace`: 200 pairs of each side at both shapes
    and nothing else; the kernels' own times are in the trace's statistics."""
    import torch
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    for n, K in ((768, 10), (256, 1000)):
        for fn in xent_pairs(n, K, dev, gen):
            for _ in range(200):
                fn()
    torch.cuda.synchronize()


def digest_part(a, emit):
    """Kernel times per launch size from the database a `rocprofv3 --kernel-trace --stats` run of `--trace` wrote."""
    import sqlite3
    db = sqlite3.connect(a.digest)
    emit('kernel trace of `--trace` (200 pairs per side and shape; us per launch, by kernel and grid size in threads):')
    q = ("select substr(name, 1, 72), grid_x, count(*), avg(end - start) / 1000.0, min(end - start) / 1000.0 from kernels "
         "where name like '%softmax%' or name like '%nll_loss%' group by 1, 2 order by 1, 2")
    for name, grid, calls, mean, low in db.execute(q):
        emit('  %-72s grid %-7d %4d launches: mean %.2f us, min %.2f us' % (name, grid, calls, mean, low))


def glyphs(num_images, noise=16.0, seed=0):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from tests.test_gpu_classifier import glyph_set
    return glyph_set(num_images, noise, seed)


def trainer_part(a, emit):
    import torch
    from inclusivegan_amd import train_classifier as TC
    images, onehot = glyphs(2048)
    _, rec = TC.train_classifier(images, onehot, minibatch=256, holdout=256, total_steps=a.steps, tick_kimg=256 * (a.steps // 3) / 1000.0,
                                 log=lambda s: emit('  ' + s))
    emit('train_classifier, digits mode, minibatch 256 (768 rows per step), fmap_base 1024, 32 x 32, eager: median %.5f s per step over the ticks '
         'of %d steps on %s (the first tick includes warm-up; whether the step is launch-bound is unmeasured)'
         % (rec['sec_per_step'], a.steps, torch.cuda.get_device_properties(0).gcnArchName))


def learning_part(a, emit):
    import torch
    import tests.test_gpu_classifier as T
    from inclusivegan_amd import train_classifier as TC
    dev = torch.device('cuda', 0)
    images, onehot = T.glyph_set(T.LEARN_IMAGES, T.NOISE)
    net = T.make_net(dev, True, 10, seed=33, bias_noise=False)
    op = T.oracle_params(net)
    _, rec = TC.train_classifier(images, onehot, mode='digits', minibatch=T.LEARN_MB, lrate=T.LEARN_LRATE, holdout=T.LEARN_HOLDOUT, seed=5,
                                 net=net, total_steps=T.LEARN_STEPS, device=dev, log=lambda s: None)
    o_err, o_rows, o_gap = T.oracle_training_run(op, images, TC.class_targets(onehot, 'digits'), T.LEARN_IMAGES - T.LEARN_HOLDOUT,
                                                 T.LEARN_STEPS, T.LEARN_MB, T.LEARN_LRATE, seed=5)
    emit('synthetic learning run: noise sigma %g, %d images (%d held out), %d steps of %d images at lrate %g: fp64 run %d errors of %d held-out '
         'planes (accuracy %.4f, smallest top-two gap %.3f), HIP run %d errors of %d (accuracy %.4f)'
         % (T.NOISE, T.LEARN_IMAGES, T.LEARN_HOLDOUT, T.LEARN_STEPS, T.LEARN_MB, T.LEARN_LRATE, o_err, o_rows, 1 - o_err / o_rows, o_gap,
            rec['holdout_errors'], rec['holdout_rows'], 1 - rec['holdout_errors'] / rec['holdout_rows']))


def mnist_part(a, emit):
    have = a.mnist_dir and os.path.isfile(os.path.join(a.mnist_dir, 'train-images-idx3-ubyte.gz'))
    if not have:
        emit('real MNIST: no files on this machine -- the held-out accuracy of the default schedule (--kimg 600 --lrate 0.002) is UNMEASURED')
        return
    import tempfile
    from inclusivegan_amd import dataset_tool, train_classifier as TC
    from inclusivegan_amd.training import dataset as dataset_mod
    with tempfile.TemporaryDirectory() as tmp:
        dataset_tool.create_mnistrgb(os.path.join(tmp, 'stacked_mnist_240k'), a.mnist_dir, num_images=240000)
        ds = dataset_mod.load_dataset(data_dir=tmp, tfrecord_dir='stacked_mnist_240k', max_label_size='full')
        _, rec = TC.train_classifier(ds._images, ds._labels, log=lambda s: emit('  ' + s))
    emit('real MNIST, default schedule: held-out digit accuracy %.4f (%d errors of %d planes)'
         % (1 - rec['holdout_errors'] / rec['holdout_rows'], rec['holdout_errors'], rec['holdout_rows']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20000)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--mnist-dir', default=None)
    ap.add_argument('--trace', action='store_true', help='only launch the kernel pairs (for a kernel trace in a run of its own)')
    ap.add_argument('--digest', default=None, metavar='DB', help='print kernel times from the results database of a kernel trace of --trace')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.trace:
        trace_part(a)
        return
    if a.digest:
        lines = []
        digest_part(a, lambda t: (print(t), lines.append(t)))
        if a.out:
            with open(a.out, 'a') as f:     # the trace is a run of its own: its digest follows the record that run wrote
                f.write('\n'.join(lines) + '\n')
        return
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('classifier_bench: softmax cross-entropy kernel pair, trainer step, synthetic learning run')
    kernel_part(a, emit)
    trainer_part(a, emit)
    learning_part(a, emit)
    mnist_part(a, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
