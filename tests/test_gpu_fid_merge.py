"""GPU: fid30k on every rank.  igan_moments_merge (csrc/moments.hip) against fp64 / extended-precision NumPy -- EQUAL on integer
rows (every quantity is an integer below 2^53, so a wrong sign of the shift difference, a transposed cross term or a dropped
n_b cannot pass), blind to the unspecified lower triangle of B, within the single-stream bound of tests/test_gpu_fid.py on
float rows merged W ways, bit-identical when repeated, one non-finite value confined to its row and column;
FeatureMoments.merge; then two ranks over gloo on GPU 0 (tests/fid_dist_worker.py): the FID metric under a process group, a
non-finite feature on one rank, and the training loop evaluating the metric on both ranks at its snapshots."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import fid_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev64(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def state_of(X, shift, dev):
    """(sum, gram) device tensors of the rows X about `shift` (igan_moments_update, one call)."""
    from inclusivegan_amd import hip_ops
    F = X.shape[1]
    s, g = torch.zeros(F, device=dev, dtype=torch.float64), torch.zeros((F, F), device=dev, dtype=torch.float64)
    hip_ops.moments_update_raw(torch.from_numpy(X).to(dev), dev64(shift, dev), s, g)
    return s, g


def merged(A, shift_a, B, shift_b, dev, spoil_b=None):
    """A's state with B's folded in -> (sum, gram) NumPy, plus B's state before and after as bytes."""
    from inclusivegan_amd import hip_ops
    s_a, g_a = state_of(A, shift_a, dev)
    s_b, g_b = state_of(B, shift_b, dev)
    if spoil_b is not None:
        spoil_b(s_b, g_b)
    before = (s_b.cpu().numpy().tobytes(), g_b.cpu().numpy().tobytes())
    hip_ops.moments_merge_raw(s_a, g_a, dev64(shift_a, dev), s_b, g_b, dev64(shift_b, dev), B.shape[0])
    after = (s_b.cpu().numpy().tobytes(), g_b.cpu().numpy().tobytes())
    return s_a.cpu().numpy(), g_a.cpu().numpy(), before, after


def upper(F):
    return np.triu(np.ones((F, F), dtype=bool))


INT_SHAPES = [(1, 1, 1), (3, 5, 17), (64, 70, 65), (257, 33, 130), (1000, 300, 130)]


@pytest.mark.parametrize('shift_b_value', [5.0, None, 'per-column'])
@pytest.mark.parametrize('n_a,n_b,F', INT_SHAPES)
def test_merge_is_exact_on_integer_rows(cuda_device, n_a, n_b, F, shift_b_value):
    """A about 3.0, B about 5.0 / about no shift / both about integer shifts that differ per column, so that dl_j != dl_k and
    a cross term with its indices exchanged cannot pass either."""
    X = O.integer_rows(n_a + n_b, F)
    A, B = X[:n_a], X[n_a:]
    shift_a = np.full(F, 3.0)
    shift_b = None if shift_b_value is None else np.full(F, 5.0)
    if shift_b_value == 'per-column':
        shift_a, shift_b = 3.0 + np.arange(F) % 4, 5.0 + (3 * np.arange(F)) % 7
    want_sum, want_gram = O.moments_fp64(X, shift_a)
    got_sum, got_gram, before, after = merged(A, shift_a, B, shift_b, cuda_device)
    up = upper(F)
    assert np.array_equal(got_sum, want_sum)
    assert np.array_equal(got_gram[up], want_gram[up])
    assert before == after                                               # B is not written


def test_merge_never_reads_the_lower_triangle_of_b(cuda_device):
    n_a, n_b, F = 64, 70, 65
    X = O.integer_rows(n_a + n_b, F)
    shift_a, shift_b = np.full(F, 3.0), np.full(F, 5.0)
    low = torch.from_numpy(np.tril(np.ones((F, F), dtype=bool), k=-1)).to(cuda_device)

    def garbage(s_b, g_b):
        g_b[low] = float('nan')

    got_sum, got_gram, before, after = merged(X[:n_a], shift_a, X[n_a:], shift_b, cuda_device, spoil_b=garbage)
    want_sum, want_gram = O.moments_fp64(X, shift_a)
    assert np.array_equal(got_sum, want_sum) and np.array_equal(got_gram[upper(F)], want_gram[upper(F)])
    assert before == after


def merge_parts(X, W, dev):
    """X cut into W parts (equal up to one row), each about its own first-rows shift, folded in order into part 0's state and
    finalized -> (mean, cov, shift of part 0)."""
    from inclusivegan_amd import hip_ops
    parts = np.array_split(X, W)
    shifts = [O.first_rows_shift(p) for p in parts]
    s, g = state_of(parts[0], shifts[0], dev)
    for p, sh in zip(parts[1:], shifts[1:]):
        s_b, g_b = state_of(p, sh, dev)
        hip_ops.moments_merge_raw(s, g, dev64(shifts[0], dev), s_b, g_b, dev64(sh, dev), p.shape[0])
    mean, cov = (t.cpu().numpy() for t in hip_ops.moments_finalize_raw(s, g, dev64(shifts[0], dev), X.shape[0]))
    return mean, cov, shifts[0]


def ratios_to_the_single_stream_bound(X, mean, cov, shift):
    """max err / bound of cov and mean against the two-pass np.longdouble statistics, with the bounds test_gpu_fid.py's
    test_finalize_meets_the_bound_and_is_symmetric holds ONE stream to: gram_bound(n, diag) / (n - 1) and EPS50 sqrt(n diag)."""
    n = X.shape[0]
    want_mean, want_cov = O.mean_cov_longdouble(X)
    diag = np.diagonal(O.moments_fp64(X, shift)[1])
    cov_bound = O.gram_bound(n, diag) / (n - 1)
    mean_bound = O.EPS50 * np.sqrt(n * diag)
    err_cov = np.abs((cov.astype(np.longdouble) - want_cov).astype(np.float64))
    err_mean = np.abs((mean.astype(np.longdouble) - want_mean).astype(np.float64))
    assert np.all(diag > 0)
    return float(np.max(err_cov / cov_bound)), float(np.max(err_mean / mean_bound))


@pytest.mark.parametrize('n,F,W', [(5000, 64, 2), (333, 50, 2), (1000, 130, 4)])
def test_merged_float_rows_meet_the_single_stream_bound(cuda_device, n, F, W):
    X = O.float_rows(n, F, seed=2 * n + F)
    mean, cov, shift = merge_parts(X, W, cuda_device)
    r_cov, r_mean = ratios_to_the_single_stream_bound(X, mean, cov, shift)
    print('(%d, %d) merged %d ways: cov err / bound max %.3e, mean err / bound max %.3e' % (n, F, W, r_cov, r_mean))
    assert r_cov <= 1.0 and r_mean <= 1.0
    assert cov.tobytes() == cov.T.copy().tobytes()
    mean2, cov2, _ = merge_parts(X, W, cuda_device)
    assert mean2.tobytes() == mean.tobytes() and cov2.tobytes() == cov.tobytes()


@pytest.mark.parametrize('poison', [float('nan'), float('inf')])
def test_one_non_finite_column_of_b_reaches_its_row_and_column_only(cuda_device, poison):
    n_a, n_b, F, j = 70, 33, 130, 64
    X = O.float_rows(n_a + n_b, F, seed=9)
    A, B = X[:n_a], X[n_a:]
    shift_a, shift_b = O.first_rows_shift(A), O.first_rows_shift(B)
    clean_sum, clean_gram, _, _ = merged(A, shift_a, B, shift_b, cuda_device)

    def spoil(s_b, g_b):
        s_b[j] = poison
        g_b[j, :] = poison

    got_sum, got_gram, _, _ = merged(A, shift_a, B, shift_b, cuda_device, spoil_b=spoil)
    up = upper(F)
    touched = np.zeros((F, F), dtype=bool)
    touched[j, :] = touched[:, j] = True
    assert not np.isfinite(got_sum[j]) and not np.any(np.isfinite(got_gram[touched & up]))
    others = np.arange(F) != j
    assert got_sum[others].tobytes() == clean_sum[others].tobytes()
    assert got_gram[up & ~touched].tobytes() == clean_gram[up & ~touched].tobytes()
    assert np.all(np.isfinite(clean_gram[up])) and np.all(np.isfinite(clean_sum))


def fed(X, dev, chunk_rows, batch):
    from inclusivegan_amd import hip_ops
    fm = hip_ops.FeatureMoments(X.shape[1], dev, chunk_rows=chunk_rows)
    for r0 in range(0, X.shape[0], batch):
        fm.update(torch.from_numpy(X[r0:r0 + batch]).to(dev))
    return fm


def test_feature_moments_merge(cuda_device):
    from inclusivegan_amd import hip_ops
    dev, F = cuda_device, 70
    X = O.float_rows(150, F, seed=4)
    A, B = X[:100], X[100:]
    # a pending, unflushed partial chunk on both sides: 100 = 64 + 36 rows and 50 rows against 64-row chunks
    a, b = fed(A, dev, 64, 25), fed(B, dev, 64, 25)
    assert a._fill == 36 and b._fill == 50 and (a.count, b.count) == (100, 50)
    b_alone = fed(B, dev, 64, 25).finalize()
    shift_a = a.shift.cpu().numpy().copy()
    assert a.merge(b) is a
    assert (a.count, b.count) == (150, 50) and a._fill == 0 and b._fill == 0
    assert a.shift.cpu().numpy().tobytes() == shift_a.tobytes()         # A's shift is kept
    mu, sigma = a.finalize()
    r_cov, r_mean = ratios_to_the_single_stream_bound(X, mu, sigma, shift_a)
    print('FeatureMoments.merge 100 + 50 rows: cov err / bound max %.3e, mean err / bound max %.3e' % (r_cov, r_mean))
    assert r_cov <= 1.0 and r_mean <= 1.0
    # the other side is unchanged and usable
    mu_b, sigma_b = b.finalize()
    assert mu_b.tobytes() == b_alone[0].tobytes() and sigma_b.tobytes() == b_alone[1].tobytes()
    b.update(torch.from_numpy(A[:7]).to(dev))
    assert b.count == 57
    # empty into full: nothing moves
    empty = hip_ops.FeatureMoments(F, dev)
    a.merge(empty)
    assert a.count == 150 and empty.count == 0
    mu2, sigma2 = a.finalize()
    assert mu2.tobytes() == mu.tobytes() and sigma2.tobytes() == sigma.tobytes()
    # full into empty: the shift is adopted (a copy, not the tensor) and the statistics are the full side's
    full = fed(B, dev, 64, 25)
    empty.merge(full)
    assert empty.count == 50 and empty.shift is not full.shift and torch.equal(empty.shift, full.shift)
    mu3, sigma3 = empty.finalize()
    assert mu3.tobytes() == b_alone[0].tobytes() and sigma3.tobytes() == b_alone[1].tobytes()
    empty.update(torch.from_numpy(A[:5]).to(dev))                        # ... and it goes on as a state of its own
    assert empty.count == 55 and full.count == 50
    with pytest.raises(ValueError):
        a.merge(hip_ops.FeatureMoments(F + 1, dev))
    with pytest.raises(ValueError):
        a.merge(a)


# ---- two ranks ---------------------------------------------------------------------------------------------------------------
def run_world2(mode, outdir, data_dir=None, cwd=ROOT, timeout=600):
    """This process plus 2 ranks of tests/fid_dist_worker.py, each started fresh and waited for; -> the ranks' records."""
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, os.path.join(ROOT, 'tests', 'fid_dist_worker.py'), mode]
    procs = [subprocess.Popen(cmd + [str(r), '2', str(port), str(outdir)] + ([str(data_dir)] if data_dir else []),
                              cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=timeout) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    return [torch.load(os.path.join(str(outdir), 'rank%d.pt' % r), weights_only=False) for r in range(2)], [so for so, _ in outs]


def test_two_ranks_evaluate_fid(cuda_device, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import fid_dist_worker as W
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.metrics import frechet_inception_distance as FM
    from inclusivegan_amd.training import misc, tfrecord
    rng = np.random.RandomState(2)
    os.makedirs(str(tmp_path / 'data' / 'reals'))
    with tfrecord.TFRecordExporter(str(tmp_path / 'data' / 'reals'), 128, print_progress=False) as tfr:
        for _ in range(128):
            tfr.add_image(rng.randint(0, 256, size=(3, 32, 32)).astype(np.uint8))
    work = tmp_path / 'work'
    work.mkdir()
    (r0, r1), stdout = run_world2('fid', tmp_path, data_dir=tmp_path / 'data', cwd=work)
    assert r0['error'] is None and r1['error'] is None
    # (c) the fourth global minibatch holds 4 images: rank 0 keeps a cut slice of it, rank 1 none
    assert (r0['real_rows'], r1['real_rows']) == (52, 48) and (r0['fake_rows'], r1['fake_rows']) == (52, 48)
    assert r0['real'].shape == r0['fake'].shape == (52, W.F) and r1['real'].shape == r1['fake'].shape == (48, W.F)
    # (a) both ranks hold the same bits
    for what in ('real', 'fake'):
        for a, b in zip(r0['stats'][what], r1['stats'][what]):
            assert a.tobytes() == b.tobytes(), what
    # (b) one process: shard 0 and shard 1 from the helper, merged in rank order
    dev = cuda_device
    Gs = W.make_gs(dev)
    dataset_args = dict(tfrecord_dir='reals', resolution=32, max_label_size=0)
    fid = W.make_fid()
    fid._configure('live-network', str(tmp_path / 'data'), dataset_args, False)
    for what in ('real', 'fake'):
        total = hip_ops.FeatureMoments(W.F, dev)
        for r in range(2):
            total.merge(fid._shard_moments(Gs, dict(is_validation=True), what, r, 2))
        assert total.count == 100
        mu, sigma = total.finalize()
        assert mu.tobytes() == r0['stats'][what][0].tobytes() and sigma.tobytes() == r0['stats'][what][1].tobytes(), what
    fid.close()
    # (d) the reals of both ranks, in slice order, are the rows the single-process metric sees
    W.reset_seen()
    (tmp_path / 'single').mkdir()
    monkeypatch.chdir(tmp_path / 'single')                              # its own cache file goes here
    single = W.make_fid()
    single.run(Gs, data_dir=str(tmp_path / 'data'), dataset_args=dataset_args, mirror_augment=False, log_results=False)
    single_real = W.rows('real', 100)
    slices = [FM.shard_slices(100, 16, r, 2) for r in range(2)]
    order, taken = [], [0, 0]
    for g in range(4):
        for r, rec in enumerate((r0, r1)):
            b, e = slices[r][g]
            order.append(rec['real'][taken[r]:taken[r] + e - b])
            taken[r] += e - b
    assert np.concatenate(order).tobytes() == single_real.tobytes()
    # (e) no fake row of rank 0 is a fake row of rank 1
    assert not (r0['fake'][:, None, :] == r1['fake'][None, :, :]).all(axis=2).any()
    assert len({row.tobytes() for row in np.concatenate([r0['fake'], r1['fake']])}) == 100
    # (f) only rank 0 reports, and its value is the host formula on the gathered rows
    assert len(r0['results']) == 1 and r1['results'] == []
    want = float(FM.fid_from_activations(np.concatenate([r0['real'], r1['real']]), np.concatenate([r0['fake'], r1['fake']])))
    print('FID over 2 ranks: %.12g, host formula on the gathered rows %.12g, rel %.2e' % (r0['results'][0], want, abs(r0['results'][0] - want) / max(1.0, abs(want))))
    assert abs(r0['results'][0] - want) <= 1e-6 * max(1.0, abs(want))
    with open(str(tmp_path / 'metric-fid_tiny.txt')) as f:
        assert len(f.read().strip().splitlines()) == 1
    assert 'fid_tiny' in stdout[0] and 'fid_tiny' not in stdout[1]      # rank 0 alone prints the line
    # (g) the reals cache: written once, by rank 0, and it holds the merged statistics
    files = os.listdir(str(work / '.stylegan2-cache'))
    assert len(files) == 1 and files[0].endswith('-fid_tiny-reals.pkl')
    assert len(r0['saves']) == 1 and r1['saves'] == [] and os.path.basename(r0['saves'][0]) == files[0]
    mu_file, sigma_file = misc.load_pkl(str(work / '.stylegan2-cache' / files[0]))
    assert mu_file.tobytes() == r0['stats']['real'][0].tobytes() and sigma_file.tobytes() == r0['stats']['real'][1].tobytes()


def test_non_finite_feature_on_one_rank_raises_on_both(cuda_device, tmp_path):
    """Rank 1's first fake minibatch carries one NaN: both workers end with FloatingPointError (caught and recorded), and both
    come back well inside the limit -- neither is left at a collective."""
    (r0, r1), _ = run_world2('fid_nan', tmp_path, timeout=300)
    for r in (r0, r1):
        assert r['error'] is not None and '1 of the 192 columns of mu of the fake features' in r['error'], r['error']
        assert r['results'] == []
    assert not np.isnan(r0['fake']).any() and np.isnan(r1['fake']).sum() == 1       # the NaN was rank 1's alone


def test_training_loop_evaluates_fid_on_both_ranks(cuda_device, tmp_path):
    """World 2, two iterations, a network snapshot at every tick with the small FID entry: one result line per snapshot, the
    replicas bit-identical across the ranks and to the same run with no metric at all (evaluating the metric moves no rank's
    training draws)."""
    with_dir, plain_dir = tmp_path / 'with', tmp_path / 'plain'
    with_dir.mkdir(); plain_dir.mkdir()
    (r0, r1), _ = run_world2('loop', with_dir, timeout=900)
    (p0, p1), _ = run_world2('loop_plain', plain_dir, timeout=900)
    snapshots = [f for f in os.listdir(str(with_dir / 'run')) if f.startswith('network-snapshot-')]
    with open(str(with_dir / 'run' / 'metric-fid_tiny.txt')) as f:
        lines = f.read().strip().splitlines()
    assert len(snapshots) >= 1 and len(lines) == len(snapshots) and all('fid_tiny' in ln for ln in lines)
    assert r0['feature_calls'] > 0 and r1['feature_calls'] > 0          # both ranks evaluated
    assert p0['feature_calls'] == 0 and not os.path.exists(str(plain_dir / 'run' / 'metric-fid_tiny.txt'))
    for k in ('G', 'D', 'Gs'):
        assert torch.equal(r0[k], r1[k]), k
        assert torch.equal(r0[k], p0[k]) and torch.equal(r1[k], p1[k]), k
        assert bool(torch.isfinite(r0[k]).all())
