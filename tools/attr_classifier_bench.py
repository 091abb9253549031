"""Measured record of the CelebA attribute classifier: the sigmoid cross-entropy kernel pair next to
torch.nn.functional.binary_cross_entropy_with_logits, the trainer's time per step, and what linear separability's sampling
loop costs per minibatch with one 40-output forward against 40 separate callables.

    python tools/attr_classifier_bench.py [--calls 20000] [--windows 5] [--steps 30] [--out profiles/attr_classifier.txt]

Part 1: forward + backward of hip_ops.SigmoidXentFn (igan_sigmoid_xent_fwd / _bwd) at [256, 40] (minibatch 256, CelebA's 40
attributes), and of F.binary_cross_entropy_with_logits(reduction='none') forward + backward on the same device tensors -- the
path a user would otherwise take; the parent tree has no such op, so there is no earlier time.  Stream time between two events
around `--calls` forward + backward pairs (a window of a second or more), the two sides alternating window by window after a
warm-up window of each, divided by the pairs: it contains whatever gap the host leaves between launches, for both sides alike.
The kernels' own times come from `rocprofv3 --kernel-trace --stats -- python tools/attr_classifier_bench.py --trace`, a run of
its own, digested with --digest.
Part 2: train_classifier's seconds per step in attributes mode at 128 x 128, minibatch 256, default width, on random images
and labels, eager.
Part 3: LS._collect per minibatch on a small 128 x 128 generator with the classifier of part 2, through classify_all (one
forward and igan_binary_probs) and through the same network injected as 40 separate callables (40 forwards and 40 torch
softmaxes), alternated window by window in one process; the ratio is measured, none is promised."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, A = 256, 40


def bce_pairs(dev, gen):
    """The two sides on the same device tensors: forward + backward of hip_ops.SigmoidXentFn and of F.binary_cross_entropy_with_logits."""
    import torch
    from inclusivegan_amd import hip_ops
    x = (torch.randn(N, A, device=dev, generator=gen) * 4).requires_grad_(True)
    t = (torch.rand(N, A, device=dev, generator=gen) < 0.3).to(torch.float32)
    w = torch.full((N, A), 1.0 / (N * A), device=dev)

    def hip_pair():
        loss, _ = hip_ops.SigmoidXentFn.apply(x, t)
        torch.autograd.grad(loss, x, w)

    def torch_pair():
        loss = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction='none')
        torch.autograd.grad(loss, x, w)

    return hip_pair, torch_pair


def alternate(sides, calls, windows, sync, clock):
    """Per-call time of every side over `windows` alternated windows of `calls` calls, after a warm-up window of each."""
    for fn in sides:
        for _ in range(calls):
            fn()
    sync()
    per = [[] for _ in sides]
    for _ in range(windows):
        for side, fn in enumerate(sides):
            per[side].append(clock(fn, calls) / calls)
    return per


def event_clock(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def wall_clock(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_part(a, emit):
    import torch
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    names = ('hip_ops.SigmoidXentFn (fp64 arithmetic, pred included)', 'torch F.binary_cross_entropy_with_logits (fp32)')
    per = alternate(bce_pairs(dev, gen), a.calls, a.windows, torch.cuda.synchronize, event_clock)
    for side, name in enumerate(names):
        us = [v * 1e6 for v in per[side]]
        emit('[%d, %d] forward + backward, %s: median %.2f us per pair, min %.2f us, max %.2f us, of %d alternated windows of %d pairs (%.2f s each; launch gaps included)'
             % (N, A, name, statistics.median(us), min(us), max(us), a.windows, a.calls, statistics.median(us) * a.calls * 1e-6))


def trace_part(a):
    """For `rocprofv3 --kernel-trace --stats -- python tools/attr_classifier_bench.py --trace`: 200 pairs of each side and
    nothing else; the kernels' own times are in the trace's statistics."""
    import torch
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    for fn in bce_pairs(dev, gen):
        for _ in range(200):
            fn()
    torch.cuda.synchronize()


def digest_part(a, emit):
    """Kernel times per launch size from the database a `rocprofv3 --kernel-trace --stats` run of `--trace` wrote: every kernel
    launched 200 times or more (the pairs; the set-up kernels run once)."""
    import sqlite3
    db = sqlite3.connect(a.digest)
    emit('kernel trace of `--trace` (200 pairs per side; us per launch, by kernel and grid size in threads):')
    q = ("select substr(name, 1, 96), grid_x, count(*), avg(end - start) / 1000.0, min(end - start) / 1000.0 from kernels "
         "group by 1, 2 having count(*) >= 200 order by 1, 2")
    for name, grid, calls, mean, low in db.execute(q):
        emit('  %-96s grid %-7d %4d launches: mean %.2f us, min %.2f us' % (name, grid, calls, mean, low))


def trainer_part(a, emit):
    import numpy as np
    import torch
    from inclusivegan_amd import train_classifier as TC
    rng = np.random.RandomState(0)
    images = rng.randint(0, 256, size=(1024, 3, 128, 128), dtype=np.uint8)
    labels = (rng.rand(1024, A) < 0.3).astype(np.float32)
    net, rec = TC.train_classifier(images, labels, mode='attributes', minibatch=256, holdout=256, total_steps=a.steps,
                                   tick_kimg=256 * (a.steps // 3) / 1000.0, log=lambda s: emit('  ' + s))
    emit('train_classifier, attributes mode, minibatch 256 (10240 pairs per step), fmap_base 1024, 128 x 128, eager, random images and labels: '
         'median %.5f s per step over the ticks of %d steps on %s (the first tick includes warm-up; the defaults of --kimg and --lrate are '
         'untested on real CelebA)' % (rec['sec_per_step'], a.steps, torch.cuda.get_device_properties(0).gcnArchName))
    return net


def collect_part(a, net, emit):
    import torch
    from inclusivegan_amd import train_classifier as TC
    from inclusivegan_amd.dnnlib import tflib
    from inclusivegan_amd.metrics import linear_separability as ls
    dev = torch.device('cuda', 0)
    Gs = tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', seed=1, num_channels=3,
                       resolution=128, label_size=0, fmap_base=1024, device=dev)
    one = TC.AttributeClassifier(net, dev)
    forty = {i: one[i] for i in range(A)}                     # a dict has no classify_all: the per-attribute torch path
    for mb in (4, 32):
        metrics = [ls.LS(num_samples=mb, num_keep=mb, attrib_indices=range(A), minibatch_per_gpu=mb, classify_fns=fns, name='ls')
                   for fns in (one, forty)]
        with torch.no_grad():
            sides = [lambda m=m: m._collect(Gs, dict(is_validation=True), mb) for m in metrics]
            per = alternate(sides, a.collect_calls, a.windows, torch.cuda.synchronize, wall_clock)
        ms = [[v * 1e3 for v in side] for side in per]
        for name, v in zip(('classify_all (one forward, igan_binary_probs)', '40 separate callables (40 forwards, 40 torch softmaxes)'), ms):
            emit('LS._collect, one minibatch of %d at 128 x 128, G forward included, %s: median %.3f ms, min %.3f ms, max %.3f ms, of %d alternated windows of %d calls (wall clock, synchronised per window)'
                 % (mb, name, statistics.median(v), min(v), max(v), a.windows, a.collect_calls))
        emit('LS._collect, minibatch %d: 40 callables / classify_all = %.2f (ratio of the medians)' % (mb, statistics.median(ms[1]) / statistics.median(ms[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20000)
    ap.add_argument('--collect-calls', type=int, default=20)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--trace', action='store_true', help='only launch the kernel pairs (for a kernel trace in a run of its own)')
    ap.add_argument('--digest', default=None, metavar='DB', help='print kernel times from the results database of a kernel trace of --trace')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.trace:
        trace_part(a)
        return
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if a.digest:
        digest_part(a, emit)
        if a.out:
            with open(a.out, 'a') as f:     # the trace is a run of its own: its digest follows the record that run wrote
                f.write('\n'.join(lines) + '\n')
        return
    emit('attr_classifier_bench: sigmoid cross-entropy kernel pair, trainer step, linear separability sampling loop')
    kernel_part(a, emit)
    net = trainer_part(a, emit)
    collect_part(a, net, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
