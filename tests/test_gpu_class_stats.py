"""GPU: the class statistics of mode_counts_24k / KL24k / is50k on the device.  igan_class_hist_update against np.argmax /
np.bincount by EQUALITY (ties, signed zeros, infinities, NaNs, odd widths, unaligned rows); igan_prob_stats_update against the
fp64 oracle of tests/class_stats_oracle.py within 1e-9 relative and bit-identical when repeated; hip_ops.SplitProbStats
against the Inception Score statement; the three metric classes on the HIP generator, device and host classifier results; the
shards of every rank rebuilt in one process; two ranks over gloo on GPU 0 (tests/class_dist_worker.py).

The 1e-9 is derived, not measured: every sum here has fewer than 2^20 fp64 operations in a fixed order, each wrong by at most
2^-53 of the running magnitude (all terms of a sum share one sign: p > 0, p log p < 0), and log is good to an ulp, so the
relative error stays below 2^20 * 2^-52 < 3e-10."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import class_stats_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9


def hist_of(x, dev, with_labels=True, counts=None):
    from inclusivegan_amd import hip_ops
    K = x.shape[1]
    counts = torch.zeros(K, device=dev, dtype=torch.int64) if counts is None else counts
    labels = torch.full((x.shape[0],), -7, device=dev, dtype=torch.int32) if with_labels else None
    hip_ops.class_hist_update_raw(torch.from_numpy(x).to(dev), counts, labels)
    return (labels.cpu().numpy() if with_labels else None), counts


@pytest.mark.parametrize('K', O.KS)
@pytest.mark.parametrize('n', O.NS)
def test_histogram_equals_numpy(cuda_device, n, K):
    x = O.logit_rows(n, K, seed=1000 * n + K)
    want_labels, want_counts = O.argmax_hist(x)
    labels, counts = hist_of(x, cuda_device)
    assert np.array_equal(labels, want_labels)
    assert np.array_equal(counts.cpu().numpy(), want_counts)


@pytest.mark.parametrize('K', [131, 1000, 1001])
def test_histogram_on_crafted_rows(cuda_device, K):
    x = O.crafted_rows(K)
    want_labels, want_counts = O.argmax_hist(x)
    # the rules themselves, so that the oracle is not taken on trust
    assert want_labels[0] == 6 and want_labels[2] == 9 and want_labels[5] == 3 and want_labels[6] == 3 and want_labels[10] == 0
    assert want_labels[12] == 77 and want_labels[13] == 3 and want_labels[15] == 90 and want_labels[16] == 90 and want_labels[-1] == K - 1
    with np.errstate(invalid='ignore'):
        labels, counts = hist_of(x, cuda_device)
    assert np.array_equal(labels, want_labels), (labels, want_labels)
    assert np.array_equal(counts.cpu().numpy(), want_counts)


@pytest.mark.parametrize('n,K', [(65, 1000), (33, 63), (16, 1001)])
def test_histogram_on_rows_that_are_only_4_byte_aligned(cuda_device, n, K):
    from inclusivegan_amd import hip_ops
    x = O.logit_rows(n, K, seed=7)
    for lead in (1, 2, 3):
        flat = torch.zeros(n * K + lead, device=cuda_device)
        flat[lead:] = torch.from_numpy(x).to(cuda_device).reshape(-1)
        view = flat[lead:].view(n, K)
        assert view.data_ptr() % 16 == 4 * lead and view.is_contiguous()
        counts = torch.zeros(K, device=cuda_device, dtype=torch.int64)
        labels = torch.empty(n, device=cuda_device, dtype=torch.int32)
        hip_ops.class_hist_update_raw(view, counts, labels)
        assert np.array_equal(labels.cpu().numpy(), np.argmax(x, 1))
        assert np.array_equal(counts.cpu().numpy(), np.bincount(np.argmax(x, 1), minlength=K))


def test_histogram_accumulates_and_takes_no_labels(cuda_device):
    from inclusivegan_amd import hip_ops
    K = 65
    parts = [O.logit_rows(n, K, seed=n) for n in (3, 257, 65)]
    counts = None
    for p in parts:
        _, counts = hist_of(p, cuda_device, with_labels=False, counts=counts)            # labels = NULL
    _, once = hist_of(np.concatenate(parts), cuda_device)
    assert torch.equal(counts, once) and int(counts.sum()) == 325
    # the class on top: float32 rows only, counts on the device, one copy at the end
    hist = hip_ops.ClassHistogram(K, cuda_device)
    for p in parts:
        hist.update(torch.from_numpy(p).to(cuda_device))
    got = hist.update(torch.from_numpy(parts[0]).to(cuda_device).t().contiguous().t(), return_labels=True)     # made contiguous
    assert np.array_equal(got.cpu().numpy(), np.argmax(parts[0], 1))
    assert hist.counts.dtype == torch.int64 and hist.counts.is_cuda and hist.count == 328
    assert np.array_equal(hist.to_host(), once.cpu().numpy() + np.bincount(np.argmax(parts[0], 1), minlength=K))
    with pytest.raises(ValueError):
        hist.update(torch.zeros(3, K, device=cuda_device, dtype=torch.float64))
    with pytest.raises(ValueError):
        hist.update(torch.zeros(3, K + 1, device=cuda_device))


def sums_of(p, dev, psum=None, plogp=None):
    from inclusivegan_amd import hip_ops
    K = p.shape[1]
    psum = torch.zeros(K, device=dev, dtype=torch.float64) if psum is None else psum
    plogp = torch.zeros(1, device=dev, dtype=torch.float64) if plogp is None else plogp
    hip_ops.prob_stats_update_raw(torch.from_numpy(p).to(dev), psum, plogp)
    return psum, plogp


@pytest.mark.parametrize('K', O.KS)
@pytest.mark.parametrize('n', O.NS)
def test_probability_sums_meet_the_bound_and_repeat_bit_for_bit(cuda_device, n, K):
    p = O.softmax_rows(n, K, seed=31 * n + K)
    q = O.softmax_rows(3, K, seed=K)
    want_psum, want_plogp = O.prob_sums(np.concatenate([p, q]))
    runs = []
    for _ in range(2):                                          # the call sequence (p, then q), twice
        psum, plogp = sums_of(p, cuda_device)
        sums_of(q, cuda_device, psum, plogp)
        runs.append((psum.cpu().numpy(), plogp.cpu().numpy()))
    (psum, plogp), again = runs
    r_psum, r_plogp = O.rel(psum, want_psum), (O.rel(plogp[0], want_plogp) if K > 1 else abs(plogp[0] - want_plogp))
    print('(%d, %d): psum rel %.3e, plogp rel %.3e' % (n, K, r_psum, r_plogp))
    assert r_psum <= BOUND and r_plogp <= BOUND                 # K = 1: every p is 1.0 and plogp an exact 0
    assert psum.tobytes() == again[0].tobytes() and plogp.tobytes() == again[1].tobytes()


def split_stats(p, S, dev, batch):
    from inclusivegan_amd import hip_ops
    stats = hip_ops.SplitProbStats(p.shape[1], p.shape[0], S, dev)
    for r0 in range(0, p.shape[0], batch):
        stats.update(torch.from_numpy(p[r0:r0 + batch]).to(dev), r0)
    return stats


@pytest.mark.parametrize('poison', [0.0, float('nan')])
def test_a_zero_or_nan_probability_reaches_its_split_only(cuda_device, poison):
    N, S, K = 30, 3, 65
    p = O.softmax_rows(N, K, seed=5)
    clean = split_stats(p, S, cuda_device, 8)
    clean_scores, clean_psum = clean.scores(), clean.psum.cpu().numpy()
    bad = p.copy()
    bad[13, 40] = poison                                        # row 13 lies in split 1 = rows [10, 20)
    stats = split_stats(bad, S, cuda_device, 8)
    scores, psum = stats.scores(), stats.psum.cpu().numpy()
    assert stats.n == [10, 10, 10]
    assert np.isnan(scores[1]) and np.isfinite(scores[0]) and np.isfinite(scores[2])
    assert scores[0] == clean_scores[0] and scores[2] == clean_scores[2]
    others = np.arange(K) != 40
    assert np.all(np.isfinite(psum[:, others])) and psum[:, others].tobytes() == clean_psum[:, others].tobytes()
    assert np.all(np.isfinite(psum[[0, 2]]))
    assert np.isnan(psum[1, 40]) == np.isnan(poison)


def test_split_prob_stats_against_inception_score_splits(cuda_device):
    from inclusivegan_amd.metrics.inception_score import inception_score_splits
    N, S, K = 50, 3, 1000                                       # splits [0, 16), [16, 33), [33, 50): batches of 8 straddle both cuts
    p = O.softmax_rows(N, K, seed=11)
    stats = split_stats(p, S, cuda_device, 8)
    assert stats.bounds == [(0, 16), (16, 33), (33, 50)] and stats.n == [16, 17, 17]
    want = O.split_scores(p, S)
    got = stats.scores()
    n, psum, plogp = O.split_sums(p, S)
    print('SplitProbStats (50, 3, 1000): scores rel %.3e, psum rel %.3e, plogp rel %.3e'
          % (O.rel(got, want), O.rel(stats.psum.cpu().numpy(), psum), O.rel(stats.plogp.cpu().numpy(), plogp)))
    assert O.rel(got, want) <= BOUND
    assert O.rel(stats.psum.cpu().numpy(), psum) <= BOUND and O.rel(stats.plogp.cpu().numpy(), plogp) <= BOUND
    # hence no further from the reference's float32 statement than that statement is from the oracle, plus the bound
    ref32 = np.asarray(inception_score_splits(p, S), dtype=np.float64)
    assert np.all(np.abs(got - ref32) <= np.abs(ref32 - want) + BOUND * np.abs(want))
    # rows in another order and another batching: the same splits
    other = split_stats(p, S, cuda_device, 50)
    assert other.n == stats.n and O.rel(other.scores(), want) <= BOUND
    with pytest.raises(ValueError):
        stats.update(torch.from_numpy(p[:8]).to(cuda_device), 45)


# ---- the metric classes ----------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _grad_mode_restored():
    was = torch.is_grad_enabled()
    yield
    torch.set_grad_enabled(was)


def worker_module():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import class_dist_worker as W
    return W


def std_close(got, want, scores):
    """np.std is 1-Lipschitz in the largest change of a score, so the bound on the scores carries over as an absolute one."""
    return abs(got - want) <= BOUND * float(np.max(np.abs(scores)))


def test_metrics_on_the_hip_generator_device_and_host_results(cuda_device):
    from inclusivegan_amd.metrics import KL as K, metric_base, mode_counts as MC
    W = worker_module()
    Gs = W.make_gs(cuda_device)
    values, seen_by = {}, {}
    for to_host in (False, True):
        seen = W.new_seen()
        group = metric_base.MetricGroup(W.metric_args(seen, num_images=20, to_host=to_host))
        torch.manual_seed(77)                                   # the same draws for both kinds of classifier
        group.run(Gs, log_results=False)
        values[to_host] = {m.name: [r.value for r in m._results] for m in group.metrics}
        seen_by[to_host] = seen
    for name in ('modes_tiny', 'kl_tiny', 'is_tiny'):
        assert len(seen_by[False][name]) == 3 and all(b.shape[0] == 8 for b in seen_by[False][name])     # 3 minibatches of 8 for 20 images
        assert np.concatenate(seen_by[False][name]).tobytes() == np.concatenate(seen_by[True][name]).tobytes()
    dev_v, host_v = values[False], values[True]
    labels_m = np.argmax(W.rows(seen_by[False]['modes_tiny'], W.K_LOGITS)[:20], axis=1)
    labels_k = np.argmax(W.rows(seen_by[False]['kl_tiny'], W.K_LOGITS)[:20], axis=1)
    assert dev_v['modes_tiny'] == host_v['modes_tiny'] == [MC.count_modes(labels_m)]
    assert dev_v['kl_tiny'] == host_v['kl_tiny'] == [K.kl_to_uniform(labels_k.astype(np.float32), W.K_LOGITS)]
    probs = W.rows(seen_by[False]['is_tiny'], W.K_PROBS)[:20]
    scores = O.split_scores(probs, W.SPLITS)
    mean, std = dev_v['is_tiny']
    print('IS on the device: mean %.15g (oracle %.15g), std %.15g (oracle %.15g)' % (mean, np.mean(scores), std, np.std(scores)))
    assert abs(mean - np.mean(scores)) <= BOUND * np.mean(scores) and std_close(std, np.std(scores), scores)
    from inclusivegan_amd.metrics.inception_score import inception_score_splits
    ref32 = inception_score_splits(probs, W.SPLITS)
    assert host_v['is_tiny'] == [np.mean(ref32), np.std(ref32)]                     # the host path is the reference's statement


def all_rows_in_global_order(per_rank_rows, num_images, mb, world):
    """The recorded rows of every rank (in the order the rank saw them) put back at their global indices."""
    from inclusivegan_amd.metrics.frechet_inception_distance import shard_slices
    K = next(r.shape[1] for r in per_rank_rows if r.shape[0])
    out = np.full((num_images, K), np.nan, dtype=np.float32)
    for rank, rws in enumerate(per_rank_rows):
        at = 0
        for b, e in shard_slices(num_images, mb, rank, world):
            out[b:e] = rws[at:at + e - b]
            at += e - b
        assert at == rws.shape[0]
    assert not np.isnan(out).any()
    return out


@pytest.mark.parametrize('world,num_images,mb,owned', [(2, 30, 8, [16, 14]), (4, 7, 3, [3, 3, 1, 0])])
def test_every_ranks_shard_rebuilt_in_one_process(cuda_device, world, num_images, mb, owned):
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.metrics import KL as K, inception_score as I, mode_counts as MC
    W = worker_module()
    Gs = W.make_gs(cuda_device)
    kwargs = dict(is_validation=True)
    torch.set_grad_enabled(False)                               # as MetricBase.run evaluates (the fixture below restores it)
    # the class histogram
    hists, logit_rows = [], []
    for rank in range(world):
        seen = []
        m = MC.mode_counts(num_images=num_images, minibatch_per_gpu=mb, classify_fn=W.make_logits_fn(seen), name='modes')
        hists.append(MC.shard_histogram(m, Gs, kwargs, rank, world))
        logit_rows.append(W.rows(seen, W.K_LOGITS))
        assert logit_rows[-1].shape[0] == owned[rank] and (hists[-1] is None) == (owned[rank] == 0)
        assert hists[-1] is None or hists[-1].count == owned[rank]
    total = hip_ops.ClassHistogram(W.K_LOGITS, cuda_device)
    for h in hists:
        if h is not None:
            total.merge(h)
    labels = np.argmax(np.concatenate(logit_rows), axis=1)
    counts = total.to_host()
    assert total.count == num_images and np.array_equal(counts, np.bincount(labels, minlength=W.K_LOGITS))
    assert MC.count_modes_from_counts(counts) == MC.count_modes(labels)
    assert K.kl_from_counts(counts) == K.kl_to_uniform(labels.astype(np.float32), W.K_LOGITS)
    # no two ranks draw the same fakes
    assert len({row.tobytes() for row in np.concatenate(logit_rows)}) == num_images
    # a rank's state is a function of (rank, world) and the arguments: built again, the same integers
    seen = []
    m = MC.mode_counts(num_images=num_images, minibatch_per_gpu=mb, classify_fn=W.make_logits_fn(seen), name='modes')
    again = MC.shard_histogram(m, Gs, kwargs, 1, world)
    assert torch.equal(again.counts, hists[1].counts) and W.rows(seen, W.K_LOGITS).tobytes() == logit_rows[1].tobytes()
    # the split sums of the Inception Score
    stats, prob_rows = [], []
    for rank in range(world):
        seen = []
        m = I.IS(num_images=num_images, num_splits=W.SPLITS, minibatch_per_gpu=mb, classify_fn=W.make_probs_fn(seen), name='is')
        stats.append(m._shard_stats(Gs, kwargs, rank, world))
        prob_rows.append(W.rows(seen, W.K_PROBS))
        assert prob_rows[-1].shape[0] == owned[rank] and (stats[-1] is None) == (owned[rank] == 0)
    merged = hip_ops.SplitProbStats(W.K_PROBS, num_images, W.SPLITS, cuda_device)
    for s in stats:
        if s is not None:
            merged.merge(s)
    p = all_rows_in_global_order(prob_rows, num_images, mb, world)
    n, psum, plogp = O.split_sums(p, W.SPLITS)
    assert merged.n == [int(v) for v in n] and sum(merged.n) == num_images
    assert O.rel(merged.psum.cpu().numpy(), psum) <= BOUND and O.rel(merged.plogp.cpu().numpy(), plogp) <= BOUND
    assert O.rel(merged.scores(), O.split_scores(p, W.SPLITS)) <= BOUND


def test_two_ranks_evaluate_the_three_metrics(cuda_device, tmp_path):
    from inclusivegan_amd.metrics import KL as K, mode_counts as MC
    W = worker_module()
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, os.path.join(ROOT, 'tests', 'class_dist_worker.py'), 'metrics']
    procs = [subprocess.Popen(cmd + [str(r), '2', str(port), str(tmp_path)], cwd=str(tmp_path), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]      # each process under its own limit
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    r0, r1 = (torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r), weights_only=False) for r in range(2))
    names = ('modes_tiny', 'kl_tiny', 'is_tiny')
    # rank 0 alone prints and writes the three lines; rank 1 ends with no results
    for name in names:
        assert name in outs[0][0] and name not in outs[1][0]
        with open(str(tmp_path / ('metric-%s.txt' % name))) as f:
            lines = f.read().strip().splitlines()
        assert len(lines) == 1 and name in lines[0]
        assert r1['results'][name] == []
        assert (r0['rows'][name].shape[0], r1['rows'][name].shape[0]) == (16, 14)          # rank 1 keeps 6 of its last 8 rows
    result_lines = [[ln for ln in so.splitlines() if ln.startswith('live-network')] for so, _ in outs]     # gloo prints a line of its own
    assert len(result_lines[0]) == 3 and result_lines[1] == []
    # the values are those of the rows both workers recorded
    for name, want_of in (('modes_tiny', lambda l: MC.count_modes(l)), ('kl_tiny', lambda l: K.kl_to_uniform(l.astype(np.float32), W.K_LOGITS))):
        labels = np.argmax(np.concatenate([r0['rows'][name], r1['rows'][name]]), axis=1)
        assert r0['results'][name] == [('', float(want_of(labels)))], name
    p = all_rows_in_global_order([r0['rows']['is_tiny'], r1['rows']['is_tiny']], W.NUM_IMAGES, W.MB, 2)
    scores = O.split_scores(p, W.SPLITS)
    (s_mean, mean), (s_std, std) = r0['results']['is_tiny']
    print('IS over 2 ranks: mean %.15g (oracle %.15g), std %.15g (oracle %.15g)' % (mean, np.mean(scores), std, np.std(scores)))
    assert (s_mean, s_std) == ('_mean', '_std')
    assert abs(mean - np.mean(scores)) <= BOUND * np.mean(scores) and std_close(std, np.std(scores), scores)
