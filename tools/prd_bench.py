"""Measured record of the PRD metric's clustering at the metric's own size (prd30k: 30 000 + 30 000 embeddings x 2 048).

Synthetic non-negative features around `--modes` centres (the evaluated set misses a fifth of them), seeded, the same on
every machine.  Two modes, because the reference's code is not present where the device is:

    python tools/prd_bench.py [--n 30000] [--dim 2048] [--runs 10] [--out FILE]
        wall time of metrics.prd_score.compute_prd_from_embedding on the device (features already resident, as PRD holds
        them), the time of one igan_kmeans_step at the batch and at the full size, and (F8, F1/8).
    python tools/prd_bench.py --reference PATH/prd_score.py [--threads 16] ...
        wall time of the reference's compute_prd_from_embedding (its functions are executed where they lie, scikit-learn's
        MiniBatchKMeans on at most --threads host threads), the CPU model, and (F8, F1/8) on the same features.

Append both outputs to profiles/prd.txt."""
import argparse
import ast
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def features(n, dim, modes, seed=0):
    rng = np.random.RandomState(seed)
    centres = (np.abs(rng.randn(modes, dim)) * 0.6).astype(np.float32)
    ref = np.abs(centres[rng.randint(0, modes, size=n)] + 0.35 * rng.randn(n, dim).astype(np.float32))
    ev = np.abs(centres[rng.randint(0, modes - modes // 5, size=n)] + 0.35 * rng.randn(n, dim).astype(np.float32))
    return ev.astype(np.float32), ref.astype(np.float32)


def cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown CPU'


def run_reference(path, ev, rf, a, emit):
    from threadpoolctl import threadpool_limits
    import sklearn
    import sklearn.cluster
    names = ('compute_prd', '_cluster_into_bins', 'compute_prd_from_embedding', '_prd_to_f_beta', 'prd_to_max_f_beta_pair')
    mod = ast.parse(open(path).read())
    m = ast.Module(body=[n for n in mod.body if isinstance(n, ast.FunctionDef) and n.name in names], type_ignores=[])
    ast.fix_missing_locations(m)
    ns = dict(np=np, sklearn=sklearn)
    exec(compile(m, '<reference prd_score>', 'exec'), ns)
    threads = min(a.threads, os.cpu_count() or 1)
    np.random.seed(a.seed)
    with threadpool_limits(limits=threads):
        t0 = time.perf_counter()
        p, r = ns['compute_prd_from_embedding'](ev, rf, num_clusters=a.clusters, num_angles=1001, num_runs=a.runs)
        dt = time.perf_counter() - t0
    f8, f18 = ns['prd_to_max_f_beta_pair'](p, r, beta=8)
    emit('reference compute_prd_from_embedding (scikit-learn %s MiniBatchKMeans, fp64 host copy %.2f GB): %.1f s wall on %d threads of %s'
         % (sklearn.__version__, 2 * ev.size * 8 / 1e9, dt, threads, cpu_model()))
    emit('reference F8 %.4f  F1/8 %.4f' % (f8, f18))


def run_device(ev, rf, a, emit):
    import torch
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.metrics import prd_score
    dev = torch.device('cuda', 0)
    evd, rfd = torch.from_numpy(ev).to(dev), torch.from_numpy(rf).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    # one step, device time only (no result leaves the device)
    X = torch.cat([evd, rfd])
    xn = hip_ops.row_sqnorm_raw(X)
    C = X[:: X.shape[0] // a.clusters][:a.clusters].contiguous()
    for rows in (1024, X.shape[0]):
        sub, subn = X[:rows], xn[:rows]
        hip_ops.kmeans_step(sub, subn, C)
        dt, _ = timed(lambda: [hip_ops.kmeans_step(sub, subn, C) for _ in range(10)])
        emit('igan_kmeans_step %6d x %d, k %d: %.3f ms per call (%.0f GB/s of X read twice)'
             % (rows, X.shape[1], a.clusters, dt / 10 * 1e3, 2 * rows * X.shape[1] * 4 / (dt / 10) / 1e9))
    del X, xn
    for rep in range(a.reps):
        dt, (p, r) = timed(lambda: prd_score.compute_prd_from_embedding(evd, rfd, num_clusters=a.clusters, num_angles=1001, num_runs=a.runs, seed=a.seed))
        f8, f18 = prd_score.prd_to_max_f_beta_pair(p, r, beta=8)
        emit('HIP compute_prd_from_embedding (%d runs, features resident, fp32): %.2f s wall (rep %d) on %s   F8 %.4f  F1/8 %.4f'
             % (a.runs, dt, rep, torch.cuda.get_device_name(0), f8, f18))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=30000)
    ap.add_argument('--dim', type=int, default=2048)
    ap.add_argument('--modes', type=int, default=50)
    ap.add_argument('--clusters', type=int, default=20)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--reference', default=None, help='path of the reference\'s prd_score.py: time it on the host instead of the device path')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('prd_bench: %d + %d x %d features, %d modes, %d clusters, %d runs' % (a.n, a.n, a.dim, a.modes, a.clusters, a.runs))
    ev, rf = features(a.n, a.dim, a.modes)
    if a.reference:
        run_reference(a.reference, ev, rf, a, emit)
    else:
        run_device(ev, rf, a, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
