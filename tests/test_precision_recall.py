"""CPU: k-NN precision / recall (pr50k3).  The golden fixture (tests/golden/pr_golden.npz, made by executing the reference's
ManifoldEstimator: tests/golden/make_pr_golden.py) agrees with an fp64 brute-force restatement of the definition; the metric
resolves from metric_defaults; the two HIP entry points validate their arguments before anything touches a device."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def load_golden():
    z = np.load(os.path.join(HERE, 'golden', 'pr_golden.npz'))
    return z, [str(c) for c in z['cases']]


def brute_sqdist(A, B, rows=16):
    """d2[i, j] = sum (A[i] - B[j])^2 in fp64, direct differences; a non-finite value counts as +inf."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    out = np.empty((A.shape[0], B.shape[0]), np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(0, A.shape[0], rows):
            d = A[i:i + rows, None, :] - B[None, :, :]
            out[i:i + rows] = (d * d).sum(2)
    out[~np.isfinite(out)] = np.inf
    return out


def brute_manifold(ref, nhood_sizes):
    """Radius = the value at 0-based position k of a point's ascending distances to all points of its set, itself included."""
    return np.sort(brute_sqdist(ref, ref), axis=1)[:, list(nhood_sizes)]


def brute_evaluate(ref, radii, ev):
    """-> predictions int32 [m, nk] (some j: d2 finite and <= radius), realism float32 [m], nearest int32 [m] (ties: lower index)."""
    d = brute_sqdist(ev, ref)
    pred = (np.isfinite(d)[:, :, None] & (d[:, :, None] <= radii[None, :, :])).any(axis=1).astype(np.int32)
    nearest = np.argmin(d, axis=1).astype(np.int32)
    with np.errstate(divide='ignore', invalid='ignore'):
        realism = (radii[nearest, 0] / d.min(axis=1)).astype(np.float32)
    return pred, realism, nearest


def test_golden_fixture_agrees_with_brute_force():
    z, cases = load_golden()
    assert cases == ['a', 'b', 'c']
    banded = 0
    for c in cases:
        ref, ev = z[c + '/ref'], z[c + '/eval']
        assert ref.dtype == np.int8 and ev.dtype == np.int8
        nhood = z[c + '/nhood_sizes'].tolist()
        radii = brute_manifold(ref, nhood)
        assert np.array_equal(radii, z[c + '/ref_radii']) and radii.max() <= 2048
        pred, realism, nearest = brute_evaluate(ref, radii, ev)
        assert np.array_equal(pred, z[c + '/precision']) and z[c + '/precision'].dtype == np.int32
        assert np.array_equal(nearest, z[c + '/nearest']) and z[c + '/nearest'].dtype == np.int32
        assert np.array_equal(realism, z[c + '/realism'], equal_nan=True) and z[c + '/realism'].dtype == np.float32
        assert np.isinf(realism).any()                                   # the exact copy: x / 0
        e_radii = brute_manifold(ev, nhood)
        assert np.array_equal(e_radii, z[c + '/eval_radii'])
        rec, _, _ = brute_evaluate(ev, e_radii, ref)
        assert np.array_equal(rec, z[c + '/recall'])
        assert np.array_equal(pred.mean(axis=0), z[c + '/knn_precision']) and np.array_equal(rec.mean(axis=0), z[c + '/knn_recall'])
        # pairs sitting exactly on a radius: `<=` matters
        assert (brute_sqdist(ev, ref)[:, :, None] == radii[None]).sum() > 0
        means = np.concatenate([pred.mean(axis=0), rec.mean(axis=0)])
        banded += bool(np.all((means > 0.2) & (means < 0.8)))
    assert banded >= 1


def test_pr50k3_resolves_to_the_pr_class():
    from inclusivegan_amd.metrics import metric_base, precision_recall
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    args = metric_defaults['pr50k3']
    assert args.func_name == 'metrics.precision_recall.PR'
    assert (args.num_images, args.nhood_size, args.minibatch_per_gpu, args.row_batch_size, args.col_batch_size) == (50000, 3, 8, 10000, 10000)
    group = metric_base.MetricGroup([args])
    m = group.metrics[0]
    assert type(m) is precision_recall.PR and m.name == 'pr50k3'
    assert (m.num_images, m.nhood_size, m.row_batch_size, m.col_batch_size) == (50000, 3, 10000, 10000)
    # the reference's surface
    for name in ('batch_pairwise_distances', 'DistanceBlock', 'ManifoldEstimator', 'knn_precision_recall_features', 'PR'):
        assert hasattr(precision_recall, name)


def test_pr_without_feature_fn_raises():
    from inclusivegan_amd.metrics import precision_recall
    m = precision_recall.PR(num_images=8, nhood_size=3, minibatch_per_gpu=4, row_batch_size=8, col_batch_size=8, name='pr8')
    with pytest.raises(RuntimeError, match=r'metrics/vgg16\.pkl'):
        m._evaluate(None, {}, 1)


def test_entry_points_validate_without_a_device():
    from inclusivegan_amd import _abi
    assert _abi.ABI_VERSION == 10
    lib = _abi.get_plugin()
    assert lib.igan_abi_version() == 10
    P = 1 << 20           # never dereferenced: validation fails first
    bad = _abi.IGAN_ERR_INVALID_ARGUMENT

    def radius(query=P, qnorm=P, cand=P, cnorm=P, kth=P, dots=P, nq=4, nc=64, dim=16, kcap=4):
        return lib.igan_knn_radius_update(None, query, qnorm, cand, cnorm, kth, dots, nq, nc, dim, kcap)

    def member(query=P, qnorm=P, cand=P, cnorm=P, radii=P, flags=P, dots=P, nq=4, nc=64, dim=16, nk=1):
        return lib.igan_manifold_member_update(None, query, qnorm, cand, cnorm, radii, flags, dots, nq, nc, dim, nk)

    for fn, bufs in ((radius, ('query', 'qnorm', 'cand', 'cnorm', 'kth', 'dots')), (member, ('query', 'qnorm', 'cand', 'cnorm', 'radii', 'flags', 'dots'))):
        for b in bufs:
            assert fn(**{b: None}) == bad, b
            assert b'null buffer' in lib.igan_last_error()
        for size in ('nq', 'nc', 'dim'):
            for v in (0, -3):
                assert fn(**{size: v}) == bad, size
                assert b'sizes must be positive' in lib.igan_last_error()
        # the 32-bit operand offsets of the product kernel: 2 GiB per operand
        assert fn(nq=1 << 20, dim=1 << 10) == bad and b'2 GiB' in lib.igan_last_error()
        assert fn(nc=1 << 20, dim=1 << 10) == bad and b'2 GiB' in lib.igan_last_error()
        assert fn(nq=1 << 16, nc=1 << 16, dim=4) == bad and b'too large' in lib.igan_last_error()
    for kcap in (0, 17, -1):
        assert radius(kcap=kcap) == bad and b'kcap' in lib.igan_last_error()
    for nk in (0, 9, -1):
        assert member(nk=nk) == bad and b'nk' in lib.igan_last_error()
    with pytest.raises(ValueError):
        _abi.check(radius(kcap=17))


def test_python_layer_has_no_cpu_path():
    import torch
    from inclusivegan_amd import hip_ops
    with pytest.raises(ValueError):
        hip_ops.knn_radius_state(4, 17, 'cpu')
    assert hip_ops.knn_radius_state(4, 4, 'cpu').shape == (4, 4)
    q = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.knn_radius_update_raw(q, torch.zeros(4), q, torch.zeros(4), hip_ops.knn_radius_state(4, 4, 'cpu'))
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.manifold_member_update_raw(q, torch.zeros(4), q, torch.zeros(4), torch.zeros(4, 1, dtype=torch.float64), torch.zeros(4, 1, dtype=torch.int32))
