"""Measured record of the batched linear SVM behind the linear separability metric at the metric's own size
(ls: n = 200 000 samples of F = 512, A = 40 attributes, 100 000 kept per attribute).

Two synthetic spaces: isotropic Gaussian samples (z-like) and anisotropic ones (w-like: a decaying spectrum and an offset);
targets from random directions with label noise, per-attribute pruning masks.  Recorded: time per gradient pass and per
Hessian-vector pass (warm-up, then the median of --reps timings of --inner back-to-back passes), bytes of X read per second
against the HBM peak of DESIGN.md, Newton iterations and pass counts of a whole fit, fit time per space, the distance
of the small test cases' solutions from their fp64 minimisers, and sklearn's LinearSVC() on ONE attribute when sklearn is there.

    python tools/ls_bench.py [--n 200000] [--dim 512] [--attribs 40] [--keep 100000] [--reps 5] [--inner 10] [--out profiles/ls_svc.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inclusivegan_amd import hip_ops                                  # noqa: E402
from inclusivegan_amd.metrics import linear_separability as LS       # noqa: E402

HBM_PEAK = 8.0e12       # HBM 8 TB/s (about 6.3 achievable)
MATRIX_PEAK = 157.3e12  # fp32 matrix instruction


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def make_space(kind, n, dim, attribs, keep, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn(n, dim, device=dev, generator=gen)
    if kind == 'w-like':
        scale = torch.exp(-3.0 * torch.arange(dim, device=dev) / dim)           # singular values over e^3
        X = X * scale + 0.5 * torch.randn(dim, device=dev, generator=gen) * scale
    t = torch.randn(dim, attribs, device=dev, generator=gen)
    s = X @ t
    s = s / s.std(dim=0, keepdim=True) + 0.5 * torch.randn(n, attribs, device=dev, generator=gen) + 0.3
    Y = torch.where(s > 0, 1, -1).to(torch.int8)
    conf = s.abs()                              # keep the most confident, as the metric does
    for a in range(attribs):
        Y[torch.argsort(conf[:, a], descending=True)[keep:], a] = 0
    return X.contiguous(), Y.contiguous()


def pass_times(X, Y, reps, inner):
    n, F = X.shape
    A = Y.shape[1]
    dev = X.device
    W = (torch.randn(A, F + 1, device=dev) / F ** 0.5).contiguous()
    dec, z = torch.empty(n, A, device=dev), torch.empty(n, A, device=dev)
    act = torch.empty(n, A, device=dev, dtype=torch.uint8)
    ws = hip_ops.linear_svc_workspace(n, F, A, dev)
    out = {}
    for name, fn in (('gradient', lambda: hip_ops.linear_svc_grad_raw(X, Y, W, dec, act, 1.0, ws)),
                     ('Hessian-vector', lambda: hip_ops.linear_svc_hv_raw(X, act, W, z, 1.0, ws))):
        for _ in range(3):
            fn()
        ts = sorted(timed(lambda: [fn() for _ in range(inner)])[0] / inner for _ in range(reps))
        out[name] = (ts[len(ts) // 2], ts[0], ts[-1])
    return out


def small_case_distances(dev):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import ls_cases
    lines = []
    for name in sorted(ls_cases.SHAPES):
        X, Y, W_star, solved = ls_cases.oracle(name)
        fit = LS.linear_svc_fit(torch.from_numpy(np.array(X)).to(dev), np.array(Y))
        d = np.linalg.norm((fit.W - W_star)[solved]) / np.linalg.norm(W_star[solved])
        lines.append('  %-16s n %5d F %4d A %3d   |W_gpu - W*| / |W*| = %.3e   Newton iterations %d..%d' %
                     ((name,) + ls_cases.SHAPES[name] + (d, fit.n_iter[solved].min(), fit.n_iter[solved].max())))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=200000)
    ap.add_argument('--dim', type=int, default=512)
    ap.add_argument('--attribs', type=int, default=40)
    ap.add_argument('--keep', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ls_svc.txt'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    lines = ['ls_bench: n %d F %d A %d keep %d  (%s)' % (a.n, a.dim, a.attribs, a.keep, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    xbytes = 4.0 * a.n * a.dim
    flops = 2 * 2.0 * a.n * a.dim * 64 * ((a.attribs + 63) // 64)         # two products per pass, 64 padded attribute columns per launch
    for kind, seed in (('z-like', 200003), ('w-like', 200009)):
        X, Y = make_space(kind, a.n, a.dim, a.attribs, a.keep, dev, seed)
        lines.append('%s samples' % kind)
        for name, (med, lo, hi) in pass_times(X, Y, a.reps, a.inner).items():
            lines.append('  %-15s pass  median %.3f ms (min %.3f max %.3f over %d x %d)   X read at %.2f TB/s = %.0f %% of the %.0f TB/s HBM peak;'
                         ' %.0f TFLOP/s = %.0f %% of the fp32 matrix peak'
                         % (name, med * 1e3, lo * 1e3, hi * 1e3, a.reps, a.inner, xbytes / med / 1e12, 100 * xbytes / med / HBM_PEAK, HBM_PEAK / 1e12,
                            flops / med / 1e12, 100 * flops / med / MATRIX_PEAK))
        LS.linear_svc_fit(X[:4096], Y[:4096], max_iter=2)          # warm-up of every kernel and torch op of the solver
        stats = {}
        t, fit = timed(lambda: LS.linear_svc_fit(X, Y, stats=stats))
        lines.append('  fit of all %d attributes: %.2f s; Newton iterations %d..%d; passes: %d gradient, %d Hessian-vector (CG + one per line search), %d line search; converged %d of %d'
                     % (a.attribs, t, fit.n_iter.min(), fit.n_iter.max(), stats['grad'], stats['hv'], stats['line'], int(fit.converged.sum()), a.attribs))
        print('\n'.join(lines[-4:]), flush=True)
        try:
            import sklearn.svm
            import warnings
            rows = (Y[:, 0] != 0).cpu().numpy()
            Xh, yh = X.cpu().numpy()[rows], Y[:, 0].cpu().numpy()[rows]
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                svm = sklearn.svm.LinearSVC().fit(Xh, yh)
            t_sk = time.perf_counter() - t0
            w_sk = np.concatenate([svm.coef_[0], svm.intercept_])
            lines.append('  sklearn LinearSVC() on attribute 0 alone, same box: %.1f s (n_iter %s); its weights lie %.3e (relative) from the HIP solve'
                         % (t_sk, svm.n_iter_, np.linalg.norm(w_sk - fit.W[0]) / np.linalg.norm(fit.W[0])))
        except ImportError:
            lines.append('  sklearn is not installed here: no LinearSVC() timing')
        print(lines[-1], flush=True)
        del X, Y
    lines.append('distance from the fp64 minimiser on the test cases (tests/ls_cases.py; bound d_ref of tests/golden/ls_golden.npz: noisy 1.439e-05, separable_wide 6.837e-03, tails 9.536e-05)')
    lines += small_case_distances(dev)
    print('\n'.join(lines[-4:]))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
