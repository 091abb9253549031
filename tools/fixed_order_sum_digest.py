#!/usr/bin/env python3
"""SHA-1 digests of the ops whose kernels sum through csrc/fixed_order_sum.h, on seeded inputs at the shapes of the benchmark
(128 x 128, 6 images per GPU; the metrics' and the classifier's row shapes), for bit-equality A/Bs of library builds whose
arithmetic must not change:
    python tools/fixed_order_sum_digest.py > a.txt; IGAN_LIB=<other libigan_hip.so> python tools/fixed_order_sum_digest.py > b.txt; diff a.txt b.txt
--reps N calls every op N times (for a kernel-trace run of the same work); the digests are those of the last call."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from inclusivegan_amd import hip_ops  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
ap.add_argument('--reps', type=int, default=1)
reps = ap.parse_args().reps
dev = torch.device('cuda', 0)
g = torch.Generator().manual_seed(11)
CL = torch.channels_last


def dig(t):
    return 'none' if t is None else hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def show(name, fn):
    for _ in range(reps):
        out = fn()
    out = out if isinstance(out, (tuple, list)) else (out,)
    print('%-44s %s' % (name, ' '.join(dig(t) for t in out)))


def randn(*shape):
    return torch.randn(*shape, generator=g).to(dev)


def act4(n, c, r):
    return randn(n, c, r, r).contiguous(memory_format=CL)


for n, c, r in [(6, 128, 128), (6, 256, 64), (6, 512, 32), (6, 512, 4), (12, 128, 128), (12, 512, 8)]:
    dy, y = act4(n, c, r), act4(n, c, r)
    noise, strength, b = randn(n, 1, r, r), randn(()), randn(c)
    s, d = torch.rand(n, c, generator=g).to(dev) + 0.5, torch.rand(n, c, generator=g).to(dev) + 0.5
    tag = '%dx%dx%d C%d' % (n, r, r, c)
    show('bias_act_noise_bwd lrelu noise  ' + tag, lambda: hip_ops.bias_act_noise_bwd_raw(dy, y, noise.reshape(-1), 3, 0.2, 2.0 ** 0.5, True))
    show('bias_act_noise_bwd linear       ' + tag, lambda: hip_ops.bias_act_noise_bwd_raw(dy, y, None, 1, 0.0, 1.0, True))
    show('bias_act_noise_bwd_dd lrelu     ' + tag, lambda: hip_ops.bias_act_noise_bwd_dd_raw(dy, y, noise, strength, b, d, 3, 0.2, 2.0 ** 0.5))
    show('bias_act_noise_bwd_dd bcast     ' + tag, lambda: hip_ops.bias_act_noise_bwd_dd_raw(dy, y, noise[:1], strength, b, d, 3, 0.2, 2.0 ** 0.5))
    show('scale_dot                       ' + tag, lambda: hip_ops.scale_dot_raw(dy, y))
    show('scale_dot scaled                ' + tag, lambda: hip_ops.scale_dot_raw(dy, y, s, want_scaled=True, keep_b=True))
    show('bias_grad rows                  ' + tag, lambda: hip_ops.bias_grad_raw(dy, c, 1))
for n, c, r in [(12, 512, 4), (6, 3, 128)]:
    x = randn(n, c, r, r)
    show('bias_grad planes                %dx%d step %d' % (n, c, r * r), lambda: hip_ops.bias_grad_raw(x, c, r * r))
for n, c, r, grp in [(12, 512, 4, 4), (12, 128, 64, 4), (6, 512, 4, 3)]:
    x, dy = act4(n, c, r), act4(n, c + 1, r)
    show('mbstd fwd / bwd                 %dx%dx%d C%d G%d' % (n, r, r, c, grp), lambda: (hip_ops.mbstd_fwd_raw(x, grp), hip_ops.mbstd_bwd_raw(x, dy, grp)))
for rows, dim in [(60, 49152), (257, 1001), (4096, 64)]:
    a = randn(rows, dim)
    show('row_sqnorm                      %d x %d' % (rows, dim), lambda: hip_ops.row_sqnorm_raw(a))
for n, K in [(32, 1000), (8, 1000), (200, 10), (67, 37)]:
    p = torch.softmax(randn(n, K), dim=1)

    def prob_stats():
        psum, plogp = torch.zeros(K, device=dev, dtype=torch.float64), torch.zeros(1, device=dev, dtype=torch.float64)
        hip_ops.prob_stats_update_raw(p, psum, plogp)
        hip_ops.prob_stats_update_raw(p, psum, plogp)
        return psum, plogp
    show('prob_stats_update x 2           %d x %d' % (n, K), prob_stats)
for n, K in [(1000, 10), (64, 10), (777, 1000)]:
    x = randn(n, K)
    labels = torch.randint(-1, K + 1, (n,), generator=g).to(torch.int32).to(dev)

    def xent():
        loss, lse, pred = hip_ops.softmax_xent_raw(x, labels)
        loss_sum, counts = torch.zeros(1, device=dev, dtype=torch.float64), torch.zeros(2, device=dev, dtype=torch.int64)
        hip_ops.xent_stats_update_raw(loss, labels, pred, loss_sum, counts, K)
        return loss, lse, pred, loss_sum, counts
    show('softmax_xent + xent_stats       %d x %d' % (n, K), xent)
