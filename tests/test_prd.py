"""CPU: the PRD metric (prd30k).  The deterministic part of metrics/prd_score.py equals the executed reference bit for bit
(tests/golden/prd_golden.npz, made by tests/golden/make_prd_golden.py), its ValueErrors are the reference's, the two HIP
exports validate their arguments before anything touches a device, the metric resolves from metric_defaults, the CLI takes
the reference's flags, and the CPU restatement of the clustering (tests/prd_oracle.py) lands inside the reference's own
seed-to-seed spread on the 12-mode fixture."""
import os

import numpy as np
import pytest

import prd_oracle

HERE = os.path.dirname(os.path.abspath(__file__))


def load_golden():
    return np.load(os.path.join(HERE, 'golden', 'prd_golden.npz'))


def reference_band(z):
    """[min - 2 std, max + 2 std] of the reference's (F8, F1/8) over its recorded seeds: from the fixture file alone."""
    return z['b/min'] - 2.0 * z['b/std'], z['b/max'] + 2.0 * z['b/std']


def PRDM():
    from inclusivegan_amd.metrics import prd_score
    return prd_score


def test_curve_and_f_beta_equal_the_executed_reference_bit_for_bit():
    prd = PRDM()
    z = load_golden()
    cases = [str(c) for c in z['a/cases']]
    assert cases == ['counts', 'disjoint', 'equal', 'random0', 'random1', 'random2']
    for c in cases:
        e, r = z['a/%s/eval_dist' % c], z['a/%s/ref_dist' % c]
        assert (e == 0).any() or c == 'counts'
        for angles in (1001, 7):
            p, rc = prd.compute_prd(e, r, num_angles=angles)
            assert p.dtype == np.float64 and p.shape == (angles,)
            assert np.array_equal(p, z['a/%s/precision%d' % (c, angles)]) and np.array_equal(rc, z['a/%s/recall%d' % (c, angles)])
            for beta in (8, 1):
                assert np.array_equal(prd._prd_to_f_beta(p, rc, beta=beta), z['a/%s/f_beta%d_%d' % (c, angles, beta)])
                pair = np.asarray(prd.prd_to_max_f_beta_pair(p, rc, beta=beta), np.float64)
                assert np.array_equal(pair, z['a/%s/max_pair%d_%d' % (c, angles, beta)])
                # the restatement the GPU trajectory test compares with is the same arithmetic
                po, ro = prd_oracle.compute_prd(e, r, num_angles=angles)
                assert np.array_equal(po, p) and np.array_equal(ro, rc)
                assert np.array_equal(np.asarray(prd_oracle.max_f_beta_pair(po, ro, beta=beta)), pair)
    # equal distributions: precision = recall = 1 somewhere; disjoint supports: nothing in common
    assert z['a/equal/max_pair1001_8'].min() > 0.999 and z['a/disjoint/max_pair1001_8'].max() == 0.0
    assert prd.prd_to_max_f_beta_pair(*prd.compute_prd(z['a/equal/eval_dist'], z['a/equal/ref_dist']))[0] > 0.999


def test_value_errors_are_the_references():
    prd = PRDM()
    z = load_golden()
    assert len(prd_oracle.ERROR_CASES) == 12
    for name, (fn, args, kwargs) in prd_oracle.ERROR_CASES.items():
        with pytest.raises(ValueError) as info:
            getattr(prd, fn)(*args, **kwargs)
        assert str(info.value) == str(z['a/errors/%s' % name]), name
    # the surface is the reference's, `plot` left out
    for name in ('compute_prd', '_cluster_into_bins', 'compute_prd_from_embedding', '_prd_to_f_beta', 'prd_to_max_f_beta_pair',
                 'minibatch_kmeans', 'PRD'):
        assert hasattr(prd, name)
    assert not hasattr(prd, 'plot')


def test_histograms_from_given_labels_equal_the_references():
    prd = PRDM()
    z = load_golden()
    for i in range(2):
        labels, ne, bins = z['a/bins%d/labels' % i], int(z['a/bins%d/num_eval' % i]), int(z['a/bins%d/num_clusters' % i])
        eb, rb = prd._bins_from_labels(labels, ne, bins)
        assert np.array_equal(eb, z['a/bins%d/eval_bins' % i]) and np.array_equal(rb, z['a/bins%d/ref_bins' % i])
        assert eb[2] == 0 and rb[2] == 0 and abs(eb.sum() - 1) < 1e-12
        eo, ro = prd_oracle.bins_from_labels(labels, ne, bins)
        assert np.allclose(eo, eb, rtol=0, atol=1e-15) and np.allclose(ro, rb, rtol=0, atol=1e-15)


def test_entry_points_validate_without_a_device():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    assert lib.igan_abi_version() == _abi.ABI_VERSION == 10          # new exports only: no bump
    P = 1 << 20           # never dereferenced: validation fails first
    bad, unsupported = _abi.IGAN_ERR_INVALID_ARGUMENT, _abi.IGAN_ERR_UNSUPPORTED
    bufs = ('X', 'xnorm', 'C', 'cnorm', 'label', 'd2', 'sums', 'count', 'inertia', 'workspace')

    def step(n=100, k=20, dim=64, **null):
        ptrs = [None if b in null else P for b in bufs]
        return lib.igan_kmeans_step(None, *ptrs, n, k, dim)

    for b in bufs:
        assert step(**{b: None}) == bad, b
        assert b'null buffer' in lib.igan_last_error()
    for n in (0, -5):
        assert step(n=n) == bad and b'n must be positive' in lib.igan_last_error()
    for k in (0, 65, -1):
        assert step(k=k) == unsupported and b'k <= 64' in lib.igan_last_error()
    for dim in (0, 4097, -1):
        assert step(dim=dim) == unsupported and b'dim <= 4096' in lib.igan_last_error()
    assert step(n=1 << 20, dim=1 << 10) == bad and b'2 GiB' in lib.igan_last_error()
    with pytest.raises(NotImplementedError):
        _abi.check(step(k=65))
    with pytest.raises(ValueError):
        _abi.check(step(n=0))
    # the workspace: 0 outside the limits, otherwise the slice partials (fp64 [slices][k][dim]) and the product block (fp32 [n][k])
    ws = lib.igan_kmeans_workspace_bytes
    for n, k, dim in ((0, 20, 64), (100, 0, 64), (100, 65, 64), (100, 20, 0), (100, 20, 4097), (1 << 20, 20, 1 << 10)):
        assert ws(n, k, dim) == 0
    assert ws(64, 1, 1) == 16 + 64 * 4                                # both parts rounded up to 16 bytes
    assert ws(1, 64, 4096) == 64 * 4096 * 8 + 64 * 4
    for n, k, dim in ((257, 1, 50), (1000, 20, 2048), (60000, 20, 2048), (5000, 64, 128)):
        got = ws(n, k, dim)
        assert got % 16 == 0 and got >= k * dim * 8 + n * k * 4
        assert (got - (n * k * 4 + 15) // 16 * 16) % (k * dim * 8) == 0
        assert ws(n, k, dim) == got                                   # a function of the sizes alone


def test_python_layer_has_no_cpu_path():
    import torch
    from inclusivegan_amd import hip_ops
    x = torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.kmeans_step_raw(x, torch.zeros(8), x[:2], torch.zeros(2))
    with pytest.raises(NotImplementedError):
        hip_ops.kmeans_step(torch.zeros(70, 4), torch.zeros(70), torch.zeros(65, 4))
    with pytest.raises(NotImplementedError):
        hip_ops.kmeans_step(torch.zeros(8, 4097), torch.zeros(8), torch.zeros(2, 4097))


def test_prd30k_resolves_to_the_prd_class():
    from inclusivegan_amd import run_metrics
    from inclusivegan_amd.metrics import metric_base, prd_score
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    args = metric_defaults['prd30k']
    assert args.func_name == 'metrics.prd_score.PRD'
    assert (args.num_images, args.num_clusters, args.num_angles, args.num_runs, args.minibatch_per_gpu) == (30000, 20, 1001, 10, 8)
    m = metric_base.MetricGroup([args]).metrics[0]
    assert type(m) is prd_score.PRD and m.name == 'prd30k' and m.feature_fn is None
    fn = lambda images: images
    injected = run_metrics._with_injected(args, dict(feature_fn=fn, classify_fn=fn))
    assert injected.get('feature_fn') is fn and 'classify_fn' not in injected


def test_prd_without_feature_fn_raises():
    from inclusivegan_amd.metrics import prd_score
    m = prd_score.PRD(num_images=8, num_clusters=2, num_angles=11, num_runs=1, minibatch_per_gpu=4, name='prd8')
    with pytest.raises(RuntimeError, match=r'PRD needs feature_fn: .*inception\.pb'):
        m._evaluate(None, {}, 1)


def test_cli_parser_takes_the_references_flags():
    from inclusivegan_amd import prd_from_image_folders as cli
    p = cli.build_parser()
    a = p.parse_args(['--reference_dir', 'real', '--eval_dirs', 'a', 'b', '--eval_labels', 'A', 'B'])
    assert (a.reference_dir, a.eval_dirs, a.eval_labels) == ('real', ['a', 'b'], ['A', 'B'])
    assert (a.num_clusters, a.num_angles, a.num_runs, a.plot_path, a.cache_dir, a.verbose) == (20, 1001, 10, None, '/tmp/prd_cache/', True)
    assert a.inception_path == 'precision-recall-distributions/inception.pb' and a.inject is None and a.seed == 0
    a = p.parse_args(['--reference_dir', 'real', '--eval_dirs', 'a', '--eval_labels', 'A', '--num_clusters', '5', '--num_angles', '101',
                      '--num_runs', '2', '--plot_path', 'x.pdf', '--cache_dir', 'c', '--inception_path', 'i.pb', '--silent',
                      '--inject', 'feature_fn=prd_oracle.box_mean_features', '--seed', '7'])
    assert (a.num_clusters, a.num_angles, a.num_runs, a.plot_path, a.cache_dir, a.inception_path, a.verbose, a.seed) == (5, 101, 2, 'x.pdf', 'c', 'i.pb', False, 7)
    assert a.inject == [('feature_fn', 'prd_oracle.box_mean_features')]
    for missing in (['--eval_dirs', 'a', '--eval_labels', 'A'], ['--reference_dir', 'r', '--eval_labels', 'A'], ['--reference_dir', 'r', '--eval_dirs', 'a']):
        with pytest.raises(SystemExit):
            p.parse_args(missing)
    with pytest.raises(ValueError, match='Number of --eval_dirs must be equal to number of --eval_labels.'):
        cli.main(['--reference_dir', 'r', '--eval_dirs', 'a', 'b', '--eval_labels', 'A'])


def test_fixture_is_the_recorded_one():
    z = load_golden()
    ev, rf = prd_oracle.mode_fixture()
    assert ev.shape == rf.shape == (1500, 64) and ev.dtype == np.float32
    assert np.array_equal(np.asarray([ev.astype(np.float64).sum(), rf.astype(np.float64).sum()]), z['b/fixture_checksum'])
    assert z['b/values'].shape[0] >= 32 and str(z['b/sklearn_version'])
    assert np.allclose(z['b/mean'], z['b/values'].mean(axis=0)) and np.allclose(z['b/std'], z['b/values'].std(axis=0, ddof=1))
    lo, hi = reference_band(z)
    assert np.all(lo < z['b/min']) and np.all(hi > z['b/max']) and np.all(hi - lo < 0.06)      # the band is narrow: a wrong partition falls outside


@pytest.mark.parametrize('seed', range(8))
def test_oracle_lies_in_the_references_band(seed):
    z = load_golden()
    lo, hi = reference_band(z)
    ev, rf = prd_oracle.mode_fixture()
    p, r = prd_oracle.compute_prd_from_embedding(ev, rf, num_clusters=20, num_angles=1001, num_runs=10, seed=seed)
    f8, f18 = prd_oracle.max_f_beta_pair(p, r, beta=8)
    print('seed %d: F8 %.5f in [%.5f, %.5f]  F1/8 %.5f in [%.5f, %.5f]' % (seed, f8, lo[0], hi[0], f18, lo[1], hi[1]))
    assert lo[0] <= f8 <= hi[0] and lo[1] <= f18 <= hi[1]


def test_oracle_step_and_kmeans_basics():
    """The restatement itself: ties to the lower index, -1 for a row without a finite distance, empty clusters, and a partition of
    well separated integer clusters that is the planted one."""
    X = np.asarray([[1, 0], [0, 0], [2, 0], [1, 5], [np.nan, 0]], np.float32)
    C = np.asarray([[0, 0], [2, 0], [2, 0], [100, 100]], np.float32)
    label, d2, sums, count, inertia = prd_oracle.brute_step(X, C)
    assert label.tolist() == [0, 0, 1, 0, -1] and d2[:4].tolist() == [1, 0, 0, 26] and np.isposinf(d2[4])
    assert count.tolist() == [3, 1, 0, 0] and np.array_equal(sums, [[2, 5], [2, 0], [0, 0], [0, 0]]) and inertia == 27
    rng = np.random.RandomState(0)
    centres = 40 * np.eye(6, 8)
    which = rng.randint(0, 6, size=400)
    data = (centres[which] + rng.randint(-2, 3, size=(400, 8))).astype(np.float32)
    labels = prd_oracle.minibatch_kmeans(data, 6, batch_size=128, rng=np.random.RandomState(1))
    assert len(set(labels.tolist())) == 6
    assert all(len(set(labels[which == m].tolist())) == 1 for m in range(6))
    with pytest.raises(ValueError, match='NaN or infinity'):
        prd_oracle.minibatch_kmeans(X, 2, rng=0)
