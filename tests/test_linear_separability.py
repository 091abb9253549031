"""CPU: the host side of linear separability (ls) and the Inception Score (is50k) against tests/golden/ls_golden.npz (the
reference's own statements and sklearn's LinearSVC, tests/golden/make_ls_golden.py); the fp64 oracle of tests/ls_cases.py
against sklearn's minimiser; the metric table rows; pruning on planted ties; the HIP entry points validate their arguments
before anything touches a device."""
import os

import numpy as np
import pytest
import torch

from tests import ls_cases
from tests.golden import make_ls_golden as gen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ls_golden.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def test_information_functions_equal_the_reference(golden):
    from inclusivegan_amd.metrics import linear_separability as ls
    tables = gen.info_tables()
    assert (tables == 0).any() and any(t[0, 1] == 0 and t[1, 0] == 0 for t in tables)      # zero cells, perfect prediction
    for k, t in enumerate(tables):
        assert np.array_equal(ls.prob_normalize(t), golden['info_prob_normalize'][k]) and ls.prob_normalize(t).dtype == np.float32
        for fn in ('mutual_information', 'entropy', 'conditional_entropy'):
            assert float(getattr(ls, fn)(t)) == golden['info_' + fn][k], (fn, k)
    assert 0.0 <= ls.conditional_entropy([[0.37, 0.0], [0.0, 0.63]]) < 1e-6          # perfect prediction: float32 noise at most
    assert (golden['info_conditional_entropy'] >= 0).all() and (golden['info_conditional_entropy'] > 0.5).any()


def test_inception_score_statistic_equals_the_reference(golden):
    from inclusivegan_amd.metrics.inception_score import inception_score_splits
    probs, splits = gen.is_probabilities()
    assert probs.shape[0] % splits != 0
    scores = inception_score_splits(probs, splits)
    assert np.array_equal(np.asarray(scores, dtype=np.float64), golden['is_scores'])
    assert np.float64(np.mean(scores)) == golden['is_mean'] and np.float64(np.std(scores)) == golden['is_std']
    assert golden['is_mean'] > 1.0 and golden['is_std'] > 0.0


@pytest.mark.parametrize('name', sorted(ls_cases.SHAPES))
def test_numpy_oracle_agrees_with_sklearn_minimiser(name, golden):
    X, Y, W, solved = ls_cases.oracle(name)
    assert X.shape == ls_cases.SHAPES[name][:2] and Y.shape == (ls_cases.SHAPES[name][0], ls_cases.SHAPES[name][2])
    tight = golden[name + '_W_tight']
    assert np.array_equal(solved, np.abs(tight).sum(axis=1) > 0)
    rel = np.linalg.norm(W - tight, axis=1)[solved] / np.linalg.norm(tight, axis=1)[solved]
    print('%s: oracle vs sklearn tol=1e-12, largest relative distance %.3e; d_ref %.3e' % (name, rel.max(), golden[name + '_d_ref']))
    assert rel.max() <= 1e-6
    assert golden[name + '_d_ref'] == golden[name + '_d_ref_dual_primal'].min() > 1e-6
    for ok, (g, rule) in zip(solved, ls_cases.stopping_rule(X, Y, W)):
        assert g <= rule or not ok


def test_tails_case_is_what_it_says():
    X, Y = ls_cases.make_case('tails')
    kept = (Y != 0).sum(axis=0)
    assert kept[ls_cases.TAILS_ALL_KEPT] == X.shape[0] and (np.delete(kept, ls_cases.TAILS_ALL_KEPT) == X.shape[0] - X.shape[0] // 2).all()
    assert (Y[:, ls_cases.TAILS_ONE_CLASS] >= 0).all()
    masks = {tuple(Y[:, a] != 0) for a in range(Y.shape[1])}
    assert len(masks) == Y.shape[1]
    assert all(d % 32 for d in X.shape) and Y.shape[1] % 32


def test_metric_table_rows_equal_the_reference():
    from inclusivegan_amd.metrics import inception_score, linear_separability, metric_base
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    ls = metric_defaults['ls']                 # metrics/metric_defaults.py:25
    assert dict(ls) == dict(name='ls', func_name='metrics.linear_separability.LS', num_samples=200000, num_keep=100000,
                            attrib_indices=range(40), minibatch_per_gpu=4)
    is50k = metric_defaults['is50k']           # :19
    assert dict(is50k) == dict(name='is50k', func_name='metrics.inception_score.IS', num_images=50000, num_splits=10, minibatch_per_gpu=8)
    a, b = metric_base.MetricGroup([ls, is50k]).metrics
    assert type(a) is linear_separability.LS and type(b) is inception_score.IS and (a.name, b.name) == ('ls', 'is50k')
    assert (a.num_samples, a.num_keep, list(a.attrib_indices), a.minibatch_per_gpu) == (200000, 100000, list(range(40)), 4)
    assert (b.num_images, b.num_splits, b.minibatch_per_gpu) == (50000, 10, 8)
    for name in ('prob_normalize', 'mutual_information', 'entropy', 'conditional_entropy', 'LS', 'linear_svc_fit', 'linear_svc_predict'):
        assert hasattr(linear_separability, name)


def test_metrics_raise_without_their_callables():
    from inclusivegan_amd.metrics import inception_score, linear_separability
    m = linear_separability.LS(num_samples=8, num_keep=4, attrib_indices=[0, 1], minibatch_per_gpu=4, name='ls8')
    with pytest.raises(RuntimeError, match=r'celebahq-classifier-00-male\.pkl'):
        m._evaluate(None, {}, 1)
    m = linear_separability.LS(num_samples=8, num_keep=4, attrib_indices=[0, 1], minibatch_per_gpu=4, classify_fns={0: None}, name='ls8')
    with pytest.raises(RuntimeError, match=r'classify_fns'):
        m._evaluate(None, {}, 1)
    m = inception_score.IS(num_images=8, num_splits=2, minibatch_per_gpu=4, name='is8')
    with pytest.raises(RuntimeError, match=r'inception_v3_softmax\.pkl'):
        m._evaluate(None, {}, 1)


def test_pruning_keeps_the_reference_set_on_planted_ties():
    """The reference sorts range(n) by -max probability with Python's stable sort and keeps the head (:153-155)."""
    from inclusivegan_amd.metrics.linear_separability import prune_most_confident, svm_targets_of
    rng = np.random.RandomState(5)
    levels = np.array([0.5, 0.625, 0.75, 0.875, 1.0], dtype=np.float32)
    hi = levels[rng.randint(0, 5, size=200)]                # many equal confidences, 0.5 / 0.5 pairs among them
    flip = rng.rand(200) < 0.5
    p = np.stack([np.where(flip, hi, 1 - hi), np.where(flip, 1 - hi, hi)], axis=1).astype(np.float32)
    for num_keep in (1, 37, 100, 200):
        want = sorted(list(range(200)), key=lambda i: -np.max(p[i]))[:num_keep]
        got = prune_most_confident(torch.from_numpy(p), num_keep).numpy()
        assert got.tolist() == want
        boundary = np.max(p[want[-1]])
        assert num_keep == 200 or (np.max(p, axis=1) == boundary).sum() > 1           # the cut runs through a tie
    assert np.array_equal(svm_targets_of(torch.from_numpy(p)).numpy(), np.argmax(p, axis=1)) and (p[:, 0] == p[:, 1]).any()


def test_entry_points_are_bound_and_validate_without_a_device():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    names = ('igan_linear_svc_workspace_bytes', 'igan_linear_svc_grad', 'igan_linear_svc_hv', 'igan_linear_svc_linesearch', 'igan_linear_svc_predict')
    for name in names:
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    assert _abi.ABI_VERSION == 10 and lib.igan_abi_version() == 10
    P = 1 << 20           # never dereferenced: validation fails first
    bad, unsupported = _abi.IGAN_ERR_INVALID_ARGUMENT, _abi.IGAN_ERR_UNSUPPORTED
    big = 1 << 40

    def grad(X=P, Y=P, W=P, dec=P, active=P, loss=P, g=P, ws=P, wsb=big, n=100, F=48, A=3, C=1.0):
        return lib.igan_linear_svc_grad(None, X, Y, W, dec, active, loss, g, ws, wsb, n, F, A, C)

    def hv(X=P, active=P, S=P, z=P, out=P, ws=P, wsb=big, n=100, F=48, A=3, C=1.0):
        return lib.igan_linear_svc_hv(None, X, active, S, z, out, ws, wsb, n, F, A, C)

    def line(dec=P, z=P, Y=P, t=P, out=P, ws=P, wsb=big, n=100, A=3, T=3):
        return lib.igan_linear_svc_linesearch(None, dec, z, Y, t, out, ws, wsb, n, A, T)

    def predict(dec=P, pred=P, n=100, A=3):
        return lib.igan_linear_svc_predict(None, dec, pred, n, A)

    buffers = {grad: ('X', 'Y', 'W', 'dec', 'active', 'loss', 'g', 'ws'), hv: ('X', 'active', 'S', 'z', 'out', 'ws'),
               line: ('dec', 'z', 'Y', 't', 'out', 'ws'), predict: ('dec', 'pred')}
    for fn, bufs in buffers.items():
        for b in bufs:
            assert fn(**{b: None}) == bad and b'null buffer' in lib.igan_last_error(), b
        for size in ('n', 'A'):
            for v in (0, -2):
                assert fn(**{size: v}) == bad and b'must be positive' in lib.igan_last_error(), size
        assert fn(n=1 << 26, A=40) == bad and b'int32' in lib.igan_last_error()            # n * A past the int32 element count
    for fn in (grad, hv, line):
        assert fn(A=65) == unsupported and b'64 attributes' in lib.igan_last_error()
        assert fn(wsb=16) == bad and b'workspace too small' in lib.igan_last_error()
    for fn in (grad, hv):
        for v in (0, -1):
            assert fn(F=v) == bad and b'F must be positive' in lib.igan_last_error()
        assert fn(F=1025) == unsupported and b'1024 features' in lib.igan_last_error()
        assert fn(n=1 << 20, F=512) == bad and b'2 GiB' in lib.igan_last_error()           # exactly 2 GiB of samples
        assert fn(C=0.0) == bad and b'C must be positive' in lib.igan_last_error()
    for T in (0, 9):
        assert line(T=T) == bad and b'T must be' in lib.igan_last_error()
    assert lib.igan_linear_svc_workspace_bytes(200000, 512, 40) > 0
    for n, F, A in ((0, 512, 40), (100, 1025, 40), (100, 512, 65), (100, 0, 1)):
        assert lib.igan_linear_svc_workspace_bytes(n, F, A) == 0
    with pytest.raises(NotImplementedError):
        _abi.check(grad(F=1025))
    with pytest.raises(ValueError):
        _abi.check(grad(n=0))


def test_python_layer_has_no_cpu_path():
    from inclusivegan_amd import hip_ops
    X, Y = torch.zeros(8, 4), torch.zeros(8, 2, dtype=torch.int8)
    W, dec, act = torch.zeros(2, 5), torch.zeros(8, 2), torch.zeros(8, 2, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.linear_svc_grad_raw(X, Y, W, dec, act)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.linear_svc_hv_raw(X, act, W, dec)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.linear_svc_linesearch_raw(dec, dec, Y, torch.zeros(3, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.linear_svc_predict_raw(dec)
