"""Measured record of the exclusive assignment's k-NN search at the CelebA-128 size (30 000 reals, 300 000 candidates of
49 152 values, k = 10), on synthetic Gaussian rows so that the search alone is timed (no generator).

Three searches, all exact, in one process:
    streaming   the shape of imle_refresh: a pack of candidates is made, folded into k (distance, index) pairs per real by
                igan_nnk_update (hip_ops.nnk_update_raw) and thrown away.  Only the folds are timed; the peak of
                torch.cuda.max_memory_allocated is the reals, ONE pack and the product block.
    resident    the path this replaces (IGAN_NNK_STREAM=0): every candidate on the device, DCI.query_device_k (torch screening,
                top-k and fp64 re-rank).  The peak includes the candidate matrix.
    1-NN        igan_nn1_update over the same rows, for scale.
Phase A runs the streaming fold and the 1-NN pack by pack with nothing resident (time and the memory peak of the streamed
shape).  Phase B puts the candidates on the device once and alternates query_device_k, query_device_nnk and query_device on the
SAME DCI object, `--reps` times: the like-for-like time comparison.  The two k-NN results are compared.

The share of (real, candidate) pairs the streaming kernel measures exactly is not counted by the kernel (it has no atomics); it
is BRACKETED by replaying the screening test in torch for `--sample` reals next to the first phase-A run: at most the pairs whose
lower bound is within U at the start of pass 2, at least those within the k-th exact distance after the batch.

Every step runs under its own time limit (SIGALRM, `--step-timeout` seconds).  A step that runs out ends the tool: nothing
more is started on the device, what was measured is written and the rest is marked "not measured".

    python tools/nnk_bench.py [--nq 30000] [--nc 300000] [--dim 49152] [--k 10] [--reps 2] [--out profiles/nnk.txt]"""
import argparse
import os
import signal
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inclusivegan_amd import hip_ops                      # noqa: E402
from inclusivegan_amd.dci_code.dci import DCI             # noqa: E402


class StepTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise StepTimeout()


def step(name, seconds, fn, log):
    """Run fn() under its own time limit -> its result, or raises StepTimeout after logging."""
    print('step: %s (limit %d s)' % (name, seconds), flush=True)
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(seconds)
    try:
        return fn()
    except StepTimeout:
        log.append('%s: NOT MEASURED (ran past its limit of %d s; the tool stopped here)' % (name, seconds))
        raise
    finally:
        signal.alarm(0)


def fill_pack(buf, pk, seed):
    g = torch.Generator(device=buf.device).manual_seed(seed + pk)
    return buf.normal_(generator=g)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bracket(qs, qn, cand, cnorm, before, after_kth, k, tol):
    """(at most, at least) pairs measured exactly for the sampled reals in this batch: the kernel's two tests replayed in torch."""
    dots = hip_ops.conv2d_raw(qs.reshape(qs.shape[0], -1, 1, 1), cand.reshape(1, 1, cand.shape[0], -1), hip_ops.ConvGeom(1, 1, 1, 1, 0, 0), (1, 1),
                              cand.shape[0], w_transposed=True).reshape(qs.shape[0], -1).double()
    s = qn.double()[:, None] + cnorm.double()[None, :]
    a, t = s - 2.0 * dots, tol * s
    u0 = torch.kthvalue(torch.cat([a + t, before], dim=1), k, dim=1).values
    return int(((a - t) <= u0[:, None]).sum()), int(((a - t) <= after_kth[:, None]).sum())


def streamed(reals, rnorm, a, dev, fold, state, seed, sample=0):
    """Phase A: packs made, folded and discarded -> (seconds of the folds, bracket counts)."""
    buf = torch.empty((min(a.pack, a.nc), a.dim), device=dev, dtype=torch.float32)
    total, hi, lo = 0.0, 0, 0
    tol = hip_ops.screening_tol(a.dim)          # nn1_tol, csrc/exact_distance.h
    k = state[0].shape[1] if state[0].dim() == 2 else 1
    for pk, c0 in enumerate(range(0, a.nc, a.pack)):
        cand = fill_pack(buf[:min(a.pack, a.nc - c0)], pk, seed)
        cnorm = hip_ops.row_sqnorm_raw(cand)
        before = state[0][:sample].clone() if sample else None

        def folds():
            for q0 in range(0, a.nq, a.query_chunk):
                fold(reals[q0:q0 + a.query_chunk], rnorm[q0:q0 + a.query_chunk], cand, cnorm, state[0][q0:q0 + a.query_chunk], state[1][q0:q0 + a.query_chunk], c0)
        dt, _ = timed(folds)
        total += dt
        if sample:
            h, l_ = bracket(reals[:sample], rnorm[:sample], cand, cnorm, before, state[0][:sample, k - 1], k, tol)
            hi += h; lo += l_
    return total, hi, lo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nq', type=int, default=30000)
    ap.add_argument('--nc', type=int, default=300000)
    ap.add_argument('--dim', type=int, default=49152)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--pack', type=int, default=4096, help='candidates per pack (imle_refresh: cand_pack)')
    ap.add_argument('--query-chunk', type=int, default=8192, help='reals per fold (imle_refresh: query_chunk)')
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--sample', type=int, default=64, help='reals whose screening is replayed for the exact-share bracket')
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--seed', type=int, default=70001)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    GB = 2.0 ** 30
    lines = ['nnk_bench: %d reals, %d candidates, dim %d, k %d, packs of %d, %d reals per fold  (%s)'
             % (a.nq, a.nc, a.dim, a.k, a.pack, a.query_chunk, torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    rc = 0
    try:
        reals = torch.empty((a.nq, a.dim), device=dev, dtype=torch.float32)
        for r0 in range(0, a.nq, a.pack):
            fill_pack(reals[r0:r0 + a.pack], r0, a.seed + (1 << 20))
        rnorm = hip_ops.row_sqnorm_raw(reals)

        def warm():      # every kernel once at a small size: code objects loaded before anything is timed
            small = argparse.Namespace(**dict(vars(a), nq=256, nc=512, pack=256, query_chunk=256))
            streamed(reals[:256], rnorm[:256], small, dev, hip_ops.nnk_update_raw, hip_ops.nnk_state(256, a.k, dev), a.seed, sample=8)
            streamed(reals[:256], rnorm[:256], small, dev, hip_ops.nn1_update_raw, hip_ops.nn1_state(256, dev), a.seed)
        step('warm-up', a.step_timeout, warm, lines)

        # ---- phase A: nothing resident
        lines.append('phase A: packs made, folded and discarded (the shape of imle_refresh); only the folds are timed')
        torch.cuda.reset_peak_memory_stats()
        state_k = hip_ops.nnk_state(a.nq, a.k, dev)
        t, hi, lo = step('A streaming k-NN', a.step_timeout, lambda: streamed(reals, rnorm, a, dev, hip_ops.nnk_update_raw, state_k, a.seed, sample=a.sample), lines)
        peak_stream = torch.cuda.max_memory_allocated()
        pairs = float(min(a.sample, a.nq)) * a.nc
        lines.append('  streaming k-NN   %8.2f s   peak memory allocated %.2f GB' % (t, peak_stream / GB))
        lines.append('  share of pairs measured exactly (bracket from a torch replay on %d reals, not counted by the kernel): between %.3e and %.3e'
                     % (min(a.sample, a.nq), lo / pairs, hi / pairs))
        torch.cuda.reset_peak_memory_stats()
        state_1 = hip_ops.nn1_state(a.nq, dev)
        t1, _, _ = step('A streaming 1-NN', a.step_timeout, lambda: streamed(reals, rnorm, a, dev, hip_ops.nn1_update_raw, state_1, a.seed), lines)
        lines.append('  streaming 1-NN   %8.2f s   peak memory allocated %.2f GB' % (t1, torch.cuda.max_memory_allocated() / GB))
        lines.append('  1-NN equals the first of the k: %s' % bool(torch.equal(state_1[1], state_k[1][:, 0]) and torch.equal(state_1[0], state_k[0][:, 0])))

        # ---- phase B: the candidates resident, the three searches alternating on one DCI object
        lines.append('phase B: every candidate resident on the device (%.1f GB), the searches alternate on the same DCI object' % (a.nc * a.dim * 4 / GB))
        torch.cuda.reset_peak_memory_stats()
        db = DCI(a.dim, device=dev)

        def make_resident():
            db._data = torch.empty((a.nc, a.dim), device=dev, dtype=torch.float32)
            for pk, c0 in enumerate(range(0, a.nc, a.pack)):
                fill_pack(db._data[c0:c0 + a.pack], pk, a.seed)
            db._norms = hip_ops.row_sqnorm_raw(db._data)
            torch.cuda.synchronize()
        step('B candidates to the device', a.step_timeout, make_resident, lines)
        times = dict(resident=[], nnk=[], nn1=[])
        res = {}
        for rep in range(a.reps):
            torch.cuda.reset_peak_memory_stats()
            t, res['resident'] = step('B resident query_device_k, rep %d' % rep, a.step_timeout, lambda: timed(lambda: db.query_device_k(reals, a.k)), lines)
            times['resident'].append(t)
            peak_resident = torch.cuda.max_memory_allocated()
            margins, thresholded = list(db.last_margins), db.last_threshold_queries
            t, res['nnk'] = step('B streaming kernel query_device_nnk, rep %d' % rep, a.step_timeout, lambda: timed(lambda: db.query_device_nnk(reals, a.k)), lines)
            times['nnk'].append(t)
            t, res['nn1'] = step('B 1-NN query_device, rep %d' % rep, a.step_timeout, lambda: timed(lambda: db.query_device(reals)), lines)
            times['nn1'].append(t)
        fmt = lambda v: ' '.join('%.2f' % x for x in v)
        lines.append('  resident  query_device_k    s per rep: %s   peak memory allocated %.2f GB   margins %s, %d reals by threshold'
                     % (fmt(times['resident']), peak_resident / GB, margins, thresholded))
        lines.append('  streaming query_device_nnk  s per rep: %s' % fmt(times['nnk']))
        lines.append('  1-NN      query_device      s per rep: %s' % fmt(times['nn1']))
        ratio = min(times['nnk']) / min(times['resident'])
        lines.append('  streaming / resident (best rep each): %.3f   streaming / 1-NN: %.3f' % (ratio, min(times['nnk']) / min(times['nn1'])))
        same_i = bool(torch.equal(res['resident'][0], res['nnk'][0]))
        err = float((res['resident'][1] - res['nnk'][1]).abs().max() / res['resident'][1].max())
        lines.append('  resident and streaming results: indices equal %s, largest distance difference %.2e of the largest distance' % (same_i, err))
        lines.append('  phase A and phase B streaming states equal: %s'
                     % bool(torch.equal(res['nnk'][0], state_k[1].to(torch.int64)) and torch.equal(res['nnk'][1], torch.sqrt(state_k[0]))))
        lines.append('memory peaks: streaming %.2f GB, resident %.2f GB' % (peak_stream / GB, peak_resident / GB))
    except StepTimeout:
        rc = 124
    for ln in lines[1:]:
        print(ln)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(rc)


if __name__ == '__main__':
    main()
