"""Measured record of the classifier metrics at their own shapes: mode_counts_24k / KL24k (24 000 images, minibatch 32, K = 1000
logits) and is50k (50 000 images, minibatch 8, 10 splits, K = 1000 probabilities).

    python tools/class_stats_bench.py [--runs 3] [--calls 2000] [--windows 5] [--skip_kernels] [--skip_metric] [--out FILE]

Part 1, the kernels (skipped on a tree that has no hip_ops.ClassHistogram): time per launch of igan_class_hist_update on
[32, 1000] logits and of igan_prob_stats_update on [8, 1000] probabilities -- stream time between two events around `--calls`
launches after a warm-up of the same launches, divided by the number of launches.  It contains whatever gap the host leaves
between launches, so it is an upper bound of the kernel's own time.

Part 2, the metrics: `--runs` complete run() calls of each of the three metrics on a small 32 x 32 generator with a stand-in
classifier on the device (a fixed random projection to 1000 columns; softmax of it for the Inception Score), with the wall time
of each and the number of device -> host copies it made (tools/fid_bench.py's counter).  This part runs unchanged on a tree
that predates the device path: run it on both and append both outputs to profiles/class_stats.txt."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 1000
SHAPES = dict(modes=(24000, 32), kl=(24000, 32), IS=(50000, 8))


def kernel_part(a, emit):
    import torch
    from inclusivegan_amd import hip_ops
    if not hasattr(hip_ops, 'ClassHistogram'):
        emit('kernels: this tree has no hip_ops.ClassHistogram (host np.argmax / activation block): part 1 skipped')
        return
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(32, K, device=dev, generator=gen)
    probs = torch.softmax(torch.randn(8, K, device=dev, generator=gen) * 3.0, dim=1)
    counts = torch.zeros(K, device=dev, dtype=torch.int64)
    psum, plogp = torch.zeros(K, device=dev, dtype=torch.float64), torch.zeros(1, device=dev, dtype=torch.float64)

    def window(fn):
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per_call.append(e0.elapsed_time(e1) / a.calls * 1e3)
        return statistics.median(per_call), min(per_call)

    med, low = window(lambda: hip_ops.class_hist_update_raw(logits, counts))
    emit('igan_class_hist_update [32, %d]: median %.2f us per launch, min %.2f us, of %d windows of %d launches (launch gaps included)'
         % (K, med, low, a.windows, a.calls))
    med, low = window(lambda: hip_ops.prob_stats_update_raw(probs, psum, plogp))
    emit('igan_prob_stats_update [8, %d]: median %.2f us per launch, min %.2f us, of %d windows of %d launches (launch gaps included)'
         % (K, med, low, a.windows, a.calls))
    probs32 = torch.softmax(torch.randn(32, K, device=dev, generator=gen) * 3.0, dim=1)
    med, low = window(lambda: hip_ops.prob_stats_update_raw(probs32, psum, plogp))
    emit('igan_prob_stats_update [32, %d]: median %.2f us per launch, min %.2f us, of %d windows of %d launches (launch gaps included)'
         % (K, med, low, a.windows, a.calls))


def metric_part(a, emit):
    import torch
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.dnnlib import tflib
    from inclusivegan_amd.metrics import KL, inception_score, mode_counts
    from tools.fid_bench import CopyCounter
    dev = torch.device('cuda', 0)
    Gs = tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', num_channels=3,
                       resolution=32, label_size=0, fmap_base=512, device=dev, seed=5)
    proj = torch.randn(3 * 32 * 32, K, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) / 8.0

    def logits_fn(images):
        return images.reshape(images.shape[0], -1) @ proj

    def probs_fn(images):
        return torch.softmax((images.to(torch.float32).reshape(images.shape[0], -1) / 255.0 - 0.5) @ proj, dim=1)

    path = 'device (hip_ops.ClassHistogram / SplitProbStats)' if hasattr(hip_ops, 'ClassHistogram') else 'host (np.argmax per minibatch / activation block)'
    emit('G 32 x 32 (fmap_base 512), classifier = fixed random projection to %d columns on the device, statistics path: %s' % (K, path))
    makers = dict(
        modes=lambda: mode_counts.mode_counts(num_images=SHAPES['modes'][0], minibatch_per_gpu=SHAPES['modes'][1], classify_fn=logits_fn, name='mode_counts_24k'),
        kl=lambda: KL.KL(num_images=SHAPES['kl'][0], minibatch_per_gpu=SHAPES['kl'][1], classify_fn=logits_fn, name='KL24k'),
        IS=lambda: inception_score.IS(num_images=SHAPES['IS'][0], num_splits=10, minibatch_per_gpu=SHAPES['IS'][1], classify_fn=probs_fn, name='is50k'))
    for key in ('modes', 'kl', 'IS'):
        walls = []
        for rep in range(a.runs):
            m = makers[key]()
            torch.cuda.synchronize()
            with CopyCounter() as copies:
                t0 = time.perf_counter()
                m.run(Gs, log_results=False)
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
            emit('  %s run %d: %.2f s wall, %d device -> host copies, %s' % (m.name, rep, walls[-1], copies.count, ', '.join('%s%s %.6f' % (m.name, r.suffix, r.value) for r in m._results)))
        emit('%s.run (%d images, minibatch %d) wall: median %.2f s, min %.2f s, max %.2f s over %d runs on %s'
             % (m.name, SHAPES[key][0], SHAPES[key][1], statistics.median(walls), min(walls), max(walls), a.runs, torch.cuda.get_device_name(0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--calls', type=int, default=2000)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--skip_kernels', action='store_true')
    ap.add_argument('--skip_metric', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('class_stats_bench: mode_counts_24k / KL24k [32, %d] per minibatch, is50k [8, %d] per minibatch' % (K, K))
    if not a.skip_kernels:
        kernel_part(a, emit)
    if not a.skip_metric:
        metric_part(a, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
