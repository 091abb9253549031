"""Measured record of the FID statistics at the metric's own size (fid30k: 30 000 features x 2 048).

    python tools/fid_bench.py [--n 30000] [--dim 2048] [--reps 3] [--runs 3] [--skip_kernels] [--skip_merge] [--skip_metric] [--out FILE]

Part 1, the kernels (skipped on a tree that has no hip_ops.FeatureMoments): the device time (events on the stream) of all
igan_moments_update launches over n resident feature rows in chunks of the metric's chunk_rows and of two other chunk sizes,
the fp64 FLOP/s they amount to, the time of igan_moments_finalize, and the largest error of cov against a two-pass
np.longdouble covariance on a sample of its rows (an extended-precision product of the whole matrix is hours of host time).

Part 1b, the merge of two states (igan_moments_merge, what FeatureMoments.all_merge runs once per rank and feature set): time
per call and bytes moved / time next to the HBM rate, cache resident and not.

Part 2, the metric: `--runs` complete FID.run calls (reals and fakes, num_images = n, the metric's minibatch of 8) on a small
32 x 32 generator with a synthetic device feature network -- a fixed random projection + ReLU to `dim` features -- with the wall
time of each and the number of device -> host copies it made (calls of Tensor.cpu / .item / .tolist / .to('cpu') on device
tensors).  This part runs unchanged on a tree that predates the device path: run it on both and append both outputs to
profiles/fid.txt."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE = 64       # MOM_TILE of csrc/moments.hip


def kernel_part(a, emit):
    import torch
    from inclusivegan_amd import hip_ops
    if not hasattr(hip_ops, 'FeatureMoments'):
        emit('kernels: this tree has no hip_ops.FeatureMoments (host np.mean / np.cov): part 1 skipped')
        return
    dev = torch.device('cuda', 0)
    n, F = a.n, a.dim
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.relu(torch.randn(n, F, device=dev, generator=gen) * torch.exp(torch.randn(n, F, device=dev, generator=gen)) + 0.3)
    shift = X[:8].double().mean(dim=0)
    tiles = (F + TILE - 1) // TILE
    flop = 2.0 * n * TILE * TILE * tiles * (tiles + 1) / 2          # 2 * n * F * (F + tile) / 2 multiply-adds when tile divides F
    emit('FLOP count: 2 * n * tile^2 * T (T + 1) / 2 with T = ceil(F / tile), tile = %d: the 64 x 64 tiles on or above the diagonal, '
         '= n * F * (F + tile) = %.3e at n = %d, F = %d' % (TILE, flop, n, F))

    def updates(chunk):
        s = torch.zeros(F, device=dev, dtype=torch.float64)
        g = torch.zeros((F, F), device=dev, dtype=torch.float64)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for r0 in range(0, n, chunk):
            hip_ops.moments_update_raw(X[r0:r0 + chunk], shift, s, g)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), s, g

    for chunk in sorted({512, hip_ops.MOMENTS_CHUNK_ROWS, 8192}):
        updates(chunk)
        ms = [updates(chunk)[0] for _ in range(a.reps)]
        med = statistics.median(ms)
        emit('igan_moments_update %d x %d in chunks of %5d rows (%3d launches)%s: median %.2f ms, min %.2f ms of %d  ->  %.1f TFLOP/s fp64'
             % (n, F, chunk, (n + chunk - 1) // chunk, ' [FeatureMoments default]' if chunk == hip_ops.MOMENTS_CHUNK_ROWS else '', med, min(ms),
                a.reps, flop / (med * 1e-3) / 1e12))
    _, s, g = updates(hip_ops.MOMENTS_CHUNK_ROWS)
    hip_ops.moments_finalize_raw(s, g, shift, n)
    ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mean, cov = hip_ops.moments_finalize_raw(s, g, shift, n)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    emit('igan_moments_finalize F = %d: median %.3f ms, min %.3f ms of %d' % (F, statistics.median(ms), min(ms), a.reps))
    rows = np.unique(np.concatenate([[0, TILE - 1, TILE, F // 2, F - 1], np.random.RandomState(0).randint(0, F, size=a.oracle_rows)]))
    rows = rows[rows < F]
    Xh = X.cpu().numpy().astype(np.longdouble)
    t0 = time.perf_counter()
    mu = Xh.sum(axis=0) / n
    C = Xh - mu[None, :]
    want = (C[:, rows].T @ C) / (n - 1)
    host_s = time.perf_counter() - t0
    got = cov.cpu().numpy()[rows].astype(np.longdouble)
    sd = np.sqrt((np.einsum('ij,ij->j', C, C) / (n - 1)).astype(np.float64))
    err = np.abs((got - want).astype(np.float64))
    emit('cov against a two-pass np.longdouble covariance, %d of its %d rows (%.1f s of host time): max |err| %.3e, max |err| / sqrt(cov_jj cov_kk) %.3e; '
         'max |mean err| %.3e' % (len(rows), F, host_s, float(err.max()), float((err / (sd[rows][:, None] * sd[None, :])).max()),
                                 float(np.max(np.abs((mean.cpu().numpy().astype(np.longdouble) - mu).astype(np.float64))))))


HBM_PEAK = 8.0e12          # bytes / s, MI355X data sheet (about 6.3e12 is what a plain copy reaches)


def merge_part(a, emit):
    """igan_moments_merge at F = dim: device time per call (events around `calls` launches, after a warm-up of the same
    launches) and bytes moved / time.  Bytes: the elements on or above the diagonal of gram_a are read and written and those
    of gram_b read, 3 * 8 * F (F + 1) / 2; sum and the shifts are 5 * 8 * F more.  Two settings: one pair of states over and
    over (50 MB at F = 2048: it stays in the 256 MB last-level cache), and `pairs` different pairs in turn, more than the cache
    holds, which is what one merge after a broadcast sees.  The time is stream time per call between two events: it includes
    whatever gap the host leaves between launches, so it is an upper bound of the kernel's own time."""
    import torch
    from inclusivegan_amd import hip_ops
    if not hasattr(hip_ops, 'moments_merge_raw'):
        emit('merge: this tree has no hip_ops.moments_merge_raw: skipped')
        return
    dev = torch.device('cuda', 0)
    F, pairs, calls = a.dim, 12, 480
    nbytes = 3 * 8 * F * (F + 1) // 2 + 5 * 8 * F
    gen = torch.Generator(device=dev).manual_seed(3)
    states = [[torch.randn(F, device=dev, dtype=torch.float64, generator=gen), torch.randn(F, F, device=dev, dtype=torch.float64, generator=gen),
               torch.randn(F, device=dev, dtype=torch.float64, generator=gen) * 1e-3] for _ in range(2 * pairs)]

    def timed(order):
        for i in order[:pairs]:
            A, B = states[2 * i], states[2 * i + 1]
            hip_ops.moments_merge_raw(A[0], A[1], A[2], B[0], B[1], B[2], 15000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in order:
            A, B = states[2 * i], states[2 * i + 1]
            hip_ops.moments_merge_raw(A[0], A[1], A[2], B[0], B[1], B[2], 15000)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / len(order)

    emit('igan_moments_merge F = %d: %.1f MB moved per call (upper triangles: gram_a read + written, gram_b read; sum, shifts)' % (F, nbytes / 1e6))
    for name, order in (('one pair repeated (cache resident)', [0] * calls), ('%d pairs in turn (%.0f MB of triangles, past the last-level cache)' % (pairs, pairs * 2 * 8 * F * (F + 1) / 2 / 1e6), [i % pairs for i in range(calls)])):
        ms = [timed(order) for _ in range(max(a.reps, 3))]
        med = sorted(ms)[len(ms) // 2]
        emit('  %s: median %.4f ms per call, min %.4f ms, of %d windows of %d calls  ->  %.2f TB/s = %.0f %% of the %.1f TB/s HBM data-sheet rate'
             % (name, med, min(ms), len(ms), calls, nbytes / (med * 1e-3) / 1e12, 100.0 * nbytes / (med * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))


class CopyCounter:
    """Counts device -> host transfers asked for through the tensor methods that make them."""

    def __init__(self):
        import torch
        self.torch, self.count, self._saved = torch, 0, {}

    def __enter__(self):
        T = self.torch.Tensor

        def wrap(name, moves):
            orig = getattr(T, name)
            self._saved[name] = orig

            def method(t, *args, **kwargs):
                if t.is_cuda and moves(args, kwargs):
                    self.count += 1
                return orig(t, *args, **kwargs)

            setattr(T, name, method)

        def to_host(args, kwargs):
            target = kwargs.get('device', args[0] if args else None)
            return isinstance(target, (str, self.torch.device)) and self.torch.device(target).type == 'cpu'

        for name in ('cpu', 'item', 'tolist'):
            wrap(name, lambda args, kwargs: True)
        wrap('to', to_host)
        return self

    def __exit__(self, *exc):
        for name, orig in self._saved.items():
            setattr(self.torch.Tensor, name, orig)


def metric_part(a, emit):
    import torch
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.dnnlib import tflib
    from inclusivegan_amd.metrics import frechet_inception_distance as FM
    dev = torch.device('cuda', 0)
    Gs = tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', num_channels=3,
                       resolution=32, label_size=0, fmap_base=512, device=dev, seed=5)
    proj = torch.randn(3 * 32 * 32, a.dim, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) / 55.0
    bias = -proj.sum(dim=0) * 100.0

    def feature_fn(images):
        return torch.relu(images.float().reshape(images.shape[0], -1) @ proj + bias)

    path = 'device (hip_ops.FeatureMoments, chunk_rows %d)' % hip_ops.MOMENTS_CHUNK_ROWS if hasattr(hip_ops, 'FeatureMoments') else 'host (np.mean / np.cov)'
    emit('FID.run: num_images %d, minibatch 8, G 32 x 32 (fmap_base 512), features relu(projection) to %d on the device, statistics path: %s'
         % (a.n, a.dim, path))
    walls = []
    for rep in range(a.runs):
        fid = FM.FID(num_images=a.n, minibatch_per_gpu=8, feature_fn=feature_fn, name='fid%dk' % (a.n // 1000))
        torch.cuda.synchronize()
        with CopyCounter() as copies:
            t0 = time.perf_counter()
            fid.run(Gs, dataset_args=dict(resolution=32, num_channels=3, label_size=0, data_size=a.n), mirror_augment=False, log_results=False)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        emit('  run %d: %.2f s wall, %d device -> host copies, FID %.6f' % (rep, walls[-1], copies.count, float(fid._results[0].value)))
    emit('FID.run wall: median %.2f s, min %.2f s, max %.2f s over %d runs (spread %.2f s) on %s'
         % (statistics.median(walls), min(walls), max(walls), a.runs, max(walls) - min(walls), torch.cuda.get_device_name(0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=30000)
    ap.add_argument('--dim', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--oracle_rows', type=int, default=12)
    ap.add_argument('--skip_kernels', action='store_true')
    ap.add_argument('--skip_metric', action='store_true')
    ap.add_argument('--skip_merge', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('fid_bench: %d x %d features' % (a.n, a.dim))
    if not a.skip_kernels:
        kernel_part(a, emit)
    if not a.skip_merge:
        merge_part(a, emit)
    if not a.skip_metric:
        metric_part(a, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
