"""Measured record of the kernel sums of the Kernel Inception Distance at the metric's own size (kid50k: 100 subsets of 1000
rows at 2048 features, drawn from 50 000 + 50 000 rows).

Synthetic non-negative features (a ReLU network's, as Inception's pool features are), the fakes a little off.  Timed, alternating
in the same repetitions of one process after a warm-up of each:

    ours        ONE igan_poly3_kernel_sums launch for all subsets (csrc/poly_kernel_sum.hip): device events around the C entry
                with the indices already on the device, and a host clock around hip_ops.poly3_kernel_sums, which also checks
                and uploads the indices
    torch fp64  the same sums as torch statements per subset: gather, .double(), three fp64 `mm`, scale, add, cube, sum

Reported besides: the achieved fp64 rate over the operations the algorithm needs (2 F per counted pair: the multiply-adds of
the dot products; the cube and the sums are not counted) and over the operations the tiles execute (padded 64 x 64 tiles,
the triangle's diagonal tiles whole); the difference of `kid` and of the three sums from (a) the brute force of
tests/kid_oracle.py on a few subsets, in units of its a-priori error budget, and (b) a torch fp32 `mm` statement of the same
sums on all subsets, which shows how many digits fp32 leaves.  Several GPUs end to end: unmeasured.

    python tools/kid_bench.py [--rows 50000] [--dim 2048] [--subsets 100] [--size 1000] [--reps 5] [--oracle-subsets 2] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from inclusivegan_amd import _abi, hip_ops                                           # noqa: E402
from inclusivegan_amd.metrics import kernel_inception_distance as KID               # noqa: E402
import kid_oracle                                                                    # noqa: E402


def torch_sums(fake, real, idx_fake, idx_real, gamma, coef0, dtype):
    """The three sums per subset as torch statements in `dtype` -> [S, 3] tensor of that type."""
    out = torch.empty((idx_fake.shape[0], 3), device=fake.device, dtype=dtype)
    for s in range(idx_fake.shape[0]):
        x, y = fake[idx_fake[s]].to(dtype), real[idx_real[s]].to(dtype)
        kxx, kyy, kxy = ((torch.mm(a, b.t()) * gamma + coef0) ** 3 for a, b in ((x, x), (y, y), (x, y)))
        out[s, 0] = kxx.sum() - torch.diagonal(kxx).sum()
        out[s, 1] = kyy.sum() - torch.diagonal(kyy).sum()
        out[s, 2] = kxy.sum()
    return out


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=50000, help='reals, and fakes')
    ap.add_argument('--dim', type=int, default=2048)
    ap.add_argument('--subsets', type=int, default=100)
    ap.add_argument('--size', type=int, default=1000, help='max_subset_size')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--oracle-subsets', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(50021)
    real = torch.relu(torch.randn(a.rows, a.dim, device=dev, generator=gen) + 0.3)
    fake = torch.relu(torch.randn(a.rows, a.dim, device=dev, generator=gen) * 1.05 + 0.32)
    idx_fake, idx_real, m = KID.kid_subsets(a.rows, a.rows, a.subsets, a.size, 0)
    S, F = a.subsets, a.dim
    gamma, coef0 = 1.0 / F, 1.0
    lines = ['kid_bench: reals %d fakes %d dim %d subsets %d of %d rows  (%s)' % (a.rows, a.rows, F, S, m, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)

    lib = _abi.get_plugin()
    nbytes = int(lib.igan_poly3_kernel_sums_workspace_bytes(S, m))
    partials = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    out = torch.empty((S, 3), device=dev, dtype=torch.float64)
    ix = torch.from_numpy(idx_fake.astype(np.int32)).to(dev)
    iy = torch.from_numpy(idx_real.astype(np.int32)).to(dev)
    jf, jr = torch.from_numpy(idx_fake).to(dev), torch.from_numpy(idx_real).to(dev)

    def entry():
        _abi.check(lib.igan_poly3_kernel_sums(hip_ops._stream(), hip_ops._ptr(fake), a.rows, hip_ops._ptr(real), a.rows, hip_ops._ptr(ix),
                                              hip_ops._ptr(iy), S, m, F, gamma, coef0, hip_ops._ptr(partials), hip_ops._ptr(out)))

    def event_timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    # warm-up of every shape the timed window uses
    entry()
    ours = hip_ops.poly3_kernel_sums(fake, real, idx_fake, idx_real, gamma, coef0)
    t64 = torch_sums(fake, real, jf, jr, gamma, coef0, torch.float64)
    torch.cuda.synchronize()
    times = dict(entry=[], binding=[], torch64=[])
    for rep in range(a.reps):
        times['entry'].append(event_timed(entry))
        t, again = host_timed(lambda: hip_ops.poly3_kernel_sums(fake, real, idx_fake, idx_real, gamma, coef0))
        times['binding'].append(t)
        t, t64 = host_timed(lambda: torch_sums(fake, real, jf, jr, gamma, coef0, torch.float64))
        times['torch64'].append(t)
        print('rep %d done' % rep, flush=True)
    same_bits = bool(torch.equal(again, ours) and torch.equal(out, ours))
    t32 = torch_sums(fake, real, jf, jr, np.float32(gamma), np.float32(coef0), torch.float32)
    ours, t64, t32 = ours.cpu().numpy(), t64.cpu().numpy(), t32.double().cpu().numpy()

    lines.append('%-44s %s' % ('pass', 'ms per rep'))
    for key, name in (('entry', 'ours: C entry, device events'), ('binding', 'ours: hip_ops call, host clock'), ('torch64', 'torch fp64 mm statement, host clock')):
        v = np.asarray(times[key]) * 1e3
        lines.append('%-44s %s   median %.3f min %.3f' % (name, ' '.join('%.3f' % t for t in v), np.median(v), v.min()))
    best = min(times['entry'])
    T = (m + 63) // 64
    needed = S * 2.0 * F * (2 * m * (m - 1) / 2 + m * m)          # each unordered pair of a symmetric sum once
    executed = S * 2.0 * F * 4096 * (T * (T + 1) + T * T)
    lines.append('fp64 rate at the best rep: %.2f TFLOP/s over the %.3e operations the sums need, %.2f TFLOP/s over the %.3e the tiles execute'
                 % (needed / best * 1e-12, needed, executed / best * 1e-12, executed))
    lines.append('ours over torch fp64 (medians, device events against host clock): %.3f'
                 % (np.median(times['entry']) / np.median(times['torch64'])))
    lines.append('every launch of ours gave the same bits: %s' % same_bits)

    kid, _ = KID.kid_from_sums(ours, m)
    kid64, _ = KID.kid_from_sums(t64, m)
    kid32, _ = KID.kid_from_sums(t32, m)
    lines.append('kid: ours %.12e   torch fp64 %.12e   torch fp32 %.12e' % (kid, kid64, kid32))
    lines.append('kid differences: torch fp64 - ours %.3e   torch fp32 - ours %.3e (%.2e of kid: fp32 leaves %.1f digits)'
                 % (kid64 - kid, kid32 - kid, abs(kid32 - kid) / abs(kid), -np.log10(abs(kid32 - kid) / abs(kid))))
    rel = lambda x: np.abs(x - ours) / np.abs(ours)
    lines.append('sums, largest relative difference from ours over all subsets (xx, yy, xy): torch fp64 %s   torch fp32 %s'
                 % (' '.join('%.2e' % v for v in rel(t64).max(axis=0)), ' '.join('%.2e' % v for v in rel(t32).max(axis=0))))
    n = max(0, min(a.oracle_subsets, S))
    if n:
        fh, rh = fake.cpu().numpy(), real.cpu().numpy()
        t0 = time.perf_counter()
        want, bound = kid_oracle.sums(fh, rh, idx_fake[:n], idx_real[:n], gamma, coef0)
        each = lambda x: np.abs(x[:n].astype(np.longdouble) - want.astype(np.longdouble)).astype(np.float64)
        lines.append('oracle (np.longdouble dots, fsum) on subsets 0 .. %d, %.0f s on the host: budget %.2e of a sum' % (n - 1, time.perf_counter() - t0, (bound / np.abs(want)).max()))
        for name, x in (('ours', ours), ('torch fp64', t64), ('torch fp32', t32)):
            lines.append('  %-10s |sum - oracle| / budget, largest over the subsets (xx, yy, xy): %s   relative: %s'
                         % (name, ' '.join('%.3g' % v for v in (each(x) / bound).max(axis=0)), ' '.join('%.2e' % v for v in (each(x) / np.abs(want)).max(axis=0))))
        okid = KID.kid_from_sums(want, m)[0]
        for name, x in (('ours', ours), ('torch fp64', t64), ('torch fp32', t32)):
            lines.append('  %-10s kid of these subsets - oracle: %.3e (budget %.2e)' % (name, KID.kid_from_sums(x[:n], m)[0] - okid, kid_oracle.kid_bound(bound, m)))
    lines.append('several GPUs end to end: unmeasured')
    for ln in lines[1:]:
        print(ln)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
