"""Measured record of the count pass of density and coverage at the metric's own size (dc50k5: 2 x 50 000 x 4 096 features, k = 5).

Synthetic Gaussian features, as tools/pr_bench.py draws them.  Timed, alternating in the same repetitions of one process:

    count       ball_counts_rows: every real against all fakes, radii of the reals (igan_ball_count_update; no early exit)
    membership  the recall pass of pr50k3 on the same operands: every real against all fakes, radii of the fakes
                (ManifoldEstimator.evaluate_rows -> manifold_member_update_raw; a marked query skips the rest).  The yardstick.
    torch       the count in a plain torch formulation: the fp32 `mm` cancellation form max(|u|^2 + |v|^2 - 2 u v^T, 0) on row
                blocks, `<` against fp32 `kthvalue` radii, `sum`

Reported besides: the number of pairs the kernel measured exactly (counted on the host from the product block the entry wrote,
with the kernel's interval arithmetic in fp64; the device may contract a multiply-add, so a pair exactly on the edge of an
interval can fall either way), and the number of count entries on which the torch form disagrees with the exact ones.

    python tools/dc_bench.py [--n 50000] [--m 50000] [--dim 4096] [--k 5] [--rows 10000] [--cols 10000] [--reps 3] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inclusivegan_amd import _abi, hip_ops                              # noqa: E402
from inclusivegan_amd.metrics import density_coverage as DC            # noqa: E402
from inclusivegan_amd.metrics import precision_recall as PR            # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def torch_radii(f, k, rows):
    n2 = (f * f).sum(1)
    out = torch.empty(f.shape[0], device=f.device, dtype=torch.float32)
    for r0 in range(0, f.shape[0], rows):
        d = torch.clamp(n2[r0:r0 + rows, None] + n2[None, :] - 2.0 * (f[r0:r0 + rows] @ f.t()), min=0.0)
        out[r0:r0 + rows] = torch.kthvalue(d, k + 1, dim=1).values
    return out


def torch_counts(real, radii, fake, rows):
    rn, fn = (real * real).sum(1), (fake * fake).sum(1)
    out = torch.empty(real.shape[0], device=real.device, dtype=torch.int64)
    for r0 in range(0, real.shape[0], rows):
        d = torch.clamp(rn[r0:r0 + rows, None] + fn[None, :] - 2.0 * (real[r0:r0 + rows] @ fake.t()), min=0.0)
        out[r0:r0 + rows] = (d < radii[r0:r0 + rows, None]).sum(dim=1)
    return out


def measured_pairs(real, radii, fake, rows, cols):
    """The count pass once more through the C entry with a product block this function owns -> (pairs the interval left to
    the exact measurement, pairs it counted as surely inside, counts): screen_interval and the two tests of
    ball_count_fold_kernel restated in fp64 on the block, for the strict comparison and one radius column."""
    lib, P, S = _abi.get_plugin(), hip_ops._ptr, hip_ops._stream()
    dim = real.shape[1]
    tol = hip_ops.screening_tol(dim)
    rn, fn = hip_ops.row_sqnorm_raw(real), hip_ops.row_sqnorm_raw(fake)
    count = hip_ops.ball_count_state(real.shape[0], 1, real.device)
    contenders = sure = 0
    for b1 in range(0, real.shape[0], rows):
        q, qn, R = real[b1:b1 + rows].contiguous(), rn[b1:b1 + rows].contiguous(), radii[b1:b1 + rows].contiguous()
        for b2 in range(0, fake.shape[0], cols):
            c, cn = fake[b2:b2 + cols].contiguous(), fn[b2:b2 + cols].contiguous()
            dots = torch.empty((q.shape[0], c.shape[0]), device=real.device, dtype=torch.float32)
            _abi.check(lib.igan_ball_count_update(S, P(q), P(qn), P(R), P(c), P(cn), P(count[b1:b1 + rows]), P(dots),
                                                  q.shape[0], c.shape[0], dim, 1, 0))
            s = qn.double()[:, None] + cn.double()[None, :]
            a = s - 2.0 * dots.double()
            s *= tol
            inside = (a + s) < R           # a finite a + t below a finite R; R [rows, 1]
            ruled_out = (a - s) >= R
            sure += int(inside.sum())
            contenders += int((~inside & ~ruled_out).sum())
            del s, a, inside, ruled_out, dots
    return contenders, sure, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=50000, help='reals')
    ap.add_argument('--m', type=int, default=50000, help='fakes')
    ap.add_argument('--dim', type=int, default=4096)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--rows', type=int, default=10000)
    ap.add_argument('--cols', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shift', type=float, default=0.02, help='mean offset of the fakes (0: both sets from one distribution)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(50003)
    real = torch.randn(a.n, a.dim, device=dev, generator=gen)
    fake = torch.randn(a.m, a.dim, device=dev, generator=gen) + a.shift
    lines = ['dc_bench: reals %d fakes %d dim %d k %d row batch %d col batch %d shift %g  (%s)'
             % (a.n, a.m, a.dim, a.k, a.rows, a.cols, a.shift, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    m_real = PR.ManifoldEstimator(None, real, a.rows, a.cols, [a.k])
    m_fake = PR.ManifoldEstimator(None, fake, a.rows, a.cols, [a.k])
    radii = torch.from_numpy(m_real.D).to(dev)
    t_radii = torch_radii(real, a.k, a.rows)
    times = {name: [] for name in ('count', 'membership', 'torch')}
    for rep in range(a.reps):
        t, counts = timed(lambda: DC.ball_counts_rows(real, radii, fake, 0, a.n, a.rows, a.cols));      times['count'].append(t)
        t, (member, _, _) = timed(lambda: m_fake.evaluate_rows(real, 0, a.n));                         times['membership'].append(t)
        t, t_counts = timed(lambda: torch_counts(real, t_radii, fake, a.rows));                        times['torch'].append(t)
        print('rep %d done' % rep, flush=True)
    contenders, sure, again = measured_pairs(real, radii, fake, a.rows, a.cols)
    counts, t_counts = counts[:, 0].cpu().numpy(), t_counts.cpu().numpy()
    lines.append('%-34s %s' % ('pass', 's per rep'))
    lines.append('%-34s %s' % ('count (igan_ball_count_update)', ' '.join('%.3f' % t for t in times['count'])))
    lines.append('%-34s %s' % ('membership, recall orientation', ' '.join('%.3f' % t for t in times['membership'])))
    lines.append('%-34s %s' % ('count, torch fp32 mm form', ' '.join('%.3f' % t for t in times['torch'])))
    best = {name: min(v) for name, v in times.items()}
    lines.append('best rep: count %.3f s, membership %.3f s: count / membership = %.3f' % (best['count'], best['membership'], best['count'] / best['membership']))
    pairs = a.n * a.m
    lines.append('pairs %d: surely inside by the interval %d, measured exactly %d (%.2e of all), ruled out %d'
                 % (pairs, sure, contenders, contenders / pairs, pairs - sure - contenders))
    lines.append('second run through the C entry gives the same counts: %s' % bool(np.array_equal(again[:, 0].cpu().numpy(), counts)))
    density, coverage = counts.sum(dtype=np.int64) / (a.k * a.m), (counts > 0).mean()
    lines.append('density %.6f coverage %.6f   torch form: density %.6f coverage %.6f   (recall of pr50k3 at this k: %.6f)'
                 % (density, coverage, t_counts.sum(dtype=np.int64) / (a.k * a.m), (t_counts > 0).mean(), float(member.float().mean())))
    lines.append('count entries the torch form gets wrong: %d of %d (reals whose coverage flips: %d)'
                 % (int((counts != t_counts).sum()), a.n, int(((counts > 0) != (t_counts > 0)).sum())))
    for ln in lines[1:]:
        print(ln)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
