"""Measured record of the k-NN precision / recall search at the metric's own size (pr50k3: 2 x 50 000 x 4 096 features, k = 3).

Synthetic Gaussian features.  The four passes of the HIP path (two manifold estimates, two membership passes; the precision
pass also asks for the nearest reference, as knn_precision_recall_features does) are timed one by one, alternating with the
same passes in a plain torch formulation in the same process: the fp32 `mm` cancellation form max(|u|^2 + |v|^2 - 2 u v^T, 0)
on row blocks, `kthvalue` for the radii and `<=` / `any` for the membership.  The number of predictions on which the two
disagree is reported (the HIP path is exact; the torch one decides near-boundary pairs by fp32 rounding).

The precision pass is timed in two forms, alternating in the same repetitions: as `evaluate` runs it, membership and nearest
neighbour on ONE product block per batch (igan_manifold_member_nn1_update), and as the pair of calls it replaced
(igan_manifold_member_update + igan_nn1_update: the product block twice).  Their results are compared bit for bit.

    python tools/pr_bench.py [--n 50000] [--dim 4096] [--k 3] [--rows 10000] [--cols 10000] [--reps 2] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inclusivegan_amd.metrics import precision_recall as PR   # noqa: E402


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


def torch_member(ref, radii, ev, rows):
    rn, en = (ref * ref).sum(1), (ev * ev).sum(1)
    out = torch.empty(ev.shape[0], device=ev.device, dtype=torch.int32)
    for r0 in range(0, ev.shape[0], rows):
        d = torch.clamp(en[r0:r0 + rows, None] + rn[None, :] - 2.0 * (ev[r0:r0 + rows] @ ref.t()), min=0.0)
        out[r0:r0 + rows] = (d <= radii[None, :]).any(dim=1).to(torch.int32)
    return out


def two_product_precision(m, ev):
    """The precision pass as the pair of calls per batch: what ManifoldEstimator.evaluate ran before the one-product entry."""
    from inclusivegan_amd import hip_ops
    dev = ev.device
    radii = torch.from_numpy(np.ascontiguousarray(m.D, dtype=np.float64)).to(dev)
    member = torch.zeros((ev.shape[0], m.num_nhoods), device=dev, dtype=torch.int32)
    best_d2, best_idx = hip_ops.nn1_state(ev.shape[0], dev)
    for b1 in range(0, ev.shape[0], m.row_batch_size):
        e1 = b1 + m.row_batch_size
        batch = ev[b1:e1]
        norms = hip_ops.row_sqnorm_raw(batch)
        for b2 in range(0, m._ref_features.shape[0], m.col_batch_size):
            e2 = b2 + m.col_batch_size
            rb, rn = m._ref_features[b2:e2], m._ref_norms[b2:e2]
            hip_ops.manifold_member_update_raw(batch, norms, rb, rn, radii[b2:e2], member[b1:e1])
            hip_ops.nn1_update_raw(batch, norms, rb, rn, best_d2[b1:e1], best_idx[b1:e1], b2)
    return m.evaluation_results(member, best_d2, best_idx, True, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=50000)
    ap.add_argument('--dim', type=int, default=4096)
    ap.add_argument('--k', type=int, default=3)
    ap.add_argument('--rows', type=int, default=10000)
    ap.add_argument('--cols', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--shift', type=float, default=0.02, help='mean offset of the evaluated set (0: both sets from one distribution)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(50003)
    ref = torch.randn(a.n, a.dim, device=dev, generator=gen)
    ev = torch.randn(a.n, a.dim, device=dev, generator=gen) + a.shift
    lines = ['pr_bench: n %d dim %d k %d row batch %d col batch %d shift %g  (%s)' % (a.n, a.dim, a.k, a.rows, a.cols, a.shift, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    hip = {name: [] for name in ('ref radii', 'eval radii', 'precision (+ nearest)', 'recall')}
    tor = {name: [] for name in hip}
    two = []
    for rep in range(a.reps):
        t, m_ref = timed(lambda: PR.ManifoldEstimator(None, ref, a.rows, a.cols, [a.k]));              hip['ref radii'].append(t)
        t, t_ref = timed(lambda: torch_radii(ref, a.k, a.rows));                                        tor['ref radii'].append(t)
        t, m_ev = timed(lambda: PR.ManifoldEstimator(None, ev, a.rows, a.cols, [a.k]));                hip['eval radii'].append(t)
        t, t_ev = timed(lambda: torch_radii(ev, a.k, a.rows));                                          tor['eval radii'].append(t)
        t, (prec, realism, nearest) = timed(lambda: m_ref.evaluate(ev, return_realism=True, return_neighbors=True)); hip['precision (+ nearest)'].append(t)
        t, t_prec = timed(lambda: torch_member(ref, t_ref, ev, a.rows));                                tor['precision (+ nearest)'].append(t)
        t, old_form = timed(lambda: two_product_precision(m_ref, ev));                                  two.append(t)
        same_bits = all(x.tobytes() == y.tobytes() for x, y in zip((prec, realism, nearest), old_form))
        t, rec = timed(lambda: m_ev.evaluate(ref));                                                     hip['recall'].append(t)
        t, t_rec = timed(lambda: torch_member(ev, t_ev, ref, a.rows));                                  tor['recall'].append(t)
        print('rep %d done' % rep, flush=True)
    lines.append('%-24s %-28s %-28s' % ('pass', 'HIP exact search, s per rep', 'torch fp32 mm form, s per rep'))
    for name in hip:
        lines.append('%-24s %-28s %-28s' % (name, ' '.join('%.3f' % t for t in hip[name]), ' '.join('%.3f' % t for t in tor[name])))
    lines.append('%-24s %-28s %-28s' % ('  as two calls, 2 products', ' '.join('%.3f' % t for t in two), '-'))
    lines.append('precision pass: one product block %.3f s, two product blocks %.3f s (best rep each); results bit-identical: %s'
                 % (min(hip['precision (+ nearest)']), min(two), same_bits))
    lines.append('%-24s %-28s %-28s' % ('total (best rep each)', '%.3f' % sum(min(v) for v in hip.values()), '%.3f' % sum(min(v) for v in tor.values())))
    t_prec, t_rec = t_prec.cpu().numpy(), t_rec.cpu().numpy()
    lines.append('knn_precision: HIP %.6f torch %.6f   knn_recall: HIP %.6f torch %.6f' % (prec.mean(), t_prec.mean(), rec.mean(), t_rec.mean()))
    lines.append('predictions that disagree: precision %d of %d, recall %d of %d' % (int((prec[:, 0] != t_prec).sum()), a.n, int((rec[:, 0] != t_rec).sum()), a.n))
    rel = np.abs(m_ref.D[:, 0] - t_ref.cpu().numpy().astype(np.float64)) / m_ref.D[:, 0]
    lines.append('radii: largest relative difference torch fp32 vs HIP exact %.3e' % rel.max())
    for ln in lines[1:]:
        print(ln)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
