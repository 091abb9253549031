"""CPU: the Kernel Inception Distance (kid50k) -- the parts that need no device.  The metric resolves from metric_defaults and
takes an injected feature network; the two entries of csrc/poly_kernel_sum.hip stand in the header, the binding and the built
library and validate their arguments before a launch; the draws of kid_subsets are pinned; kid_from_sums is the published
estimator."""
import ctypes
import os
import re

import numpy as np
import pytest

import kid_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def KIDM():
    from inclusivegan_amd.metrics import kernel_inception_distance
    return kernel_inception_distance


def test_kid50k_resolves_to_the_kid_class():
    from inclusivegan_amd.metrics import metric_base
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    import inclusivegan_amd.metrics.metric_defaults as table
    args = metric_defaults['kid50k']
    assert args.func_name == 'metrics.kernel_inception_distance.KID'
    assert (args.num_images, args.num_subsets, args.max_subset_size, args.minibatch_per_gpu) == (50000, 100, 1000, 8)
    m = metric_base.MetricGroup([args]).metrics[0]
    assert type(m) is KIDM().KID and m.name == 'kid50k'
    assert (m.num_images, m.num_subsets, m.max_subset_size, m.minibatch_per_gpu, m.seed) == (50000, 100, 1000, 8, 0)
    assert KIDM().KID.multi_rank is True
    assert 'kid50k' in table.__doc__
    assert 'choice(num_fake, m, replace=False)' in KIDM().__doc__ and 'UNBIASED' in KIDM().__doc__      # the draw order is stated


def test_kid_without_feature_fn_raises():
    m = KIDM().KID(num_images=8, num_subsets=2, max_subset_size=4, minibatch_per_gpu=4, name='kid8')
    with pytest.raises(RuntimeError, match='KID needs feature_fn'):
        m._evaluate(None, {}, 1)


def test_injected_feature_fn_reaches_the_metric():
    from inclusivegan_amd import run_metrics
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults

    def fn(images):
        return images

    args = run_metrics._with_injected(metric_defaults['kid50k'], {'feature_fn': fn, 'classify_fn': fn})
    assert args.get('feature_fn') is fn and 'classify_fn' not in args
    assert 'feature_fn' not in metric_defaults['kid50k']


def test_header_binding_and_library_carry_the_new_entries():
    from inclusivegan_amd import _abi
    header = open(os.path.join(ROOT, 'include', 'igan_hip.h')).read()
    m = re.search(r'\bint\s+igan_poly3_kernel_sums\s*\(([^;]*)\)\s*;', header)
    assert m is not None
    params = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')
    assert [p.split()[-1].lstrip('*') for p in params] == ['stream', 'X', 'nx', 'Y', 'ny', 'idx_x', 'idx_y', 'S', 'm', 'F', 'gamma', 'coef0',
                                                          'partials', 'out']
    assert 'double* partials' in m.group(1) and 'double* out' in m.group(1) and 'const int* idx_x' in m.group(1)
    assert re.search(r'\bsize_t\s+igan_poly3_kernel_sums_workspace_bytes\s*\(\s*int S\s*,\s*int m\s*\)\s*;', header)
    lib = _abi.get_plugin()
    fn, query = lib.igan_poly3_kernel_sums, lib.igan_poly3_kernel_sums_workspace_bytes
    assert len(fn.argtypes) == len(params) == 14 and fn.restype is ctypes.c_int
    assert list(fn.argtypes[10:12]) == [ctypes.c_double] * 2 and list(fn.argtypes[7:10]) == [ctypes.c_int] * 3
    assert query.restype is ctypes.c_size_t and list(query.argtypes) == [ctypes.c_int] * 2
    assert _abi.ABI_VERSION == 10 and lib.igan_abi_version() == 10
    assert re.search(r'#define\s+IGAN_ABI_VERSION\s+10\b', header)
    note = re.search(r'added under 10 without a bump.*?\*/', header, flags=re.S).group(0)
    assert 'igan_poly3_kernel_sums_workspace_bytes' in note and 'igan_poly3_kernel_sums)' in note
    assert 'NOT RANGE-CHECKED' in header                     # the caller of the C ABI owns the index check


def test_workspace_query():
    from inclusivegan_amd import _abi
    query = _abi.get_plugin().igan_poly3_kernel_sums_workspace_bytes
    # T = ceil(m / 64) tile rows: two triangles of T (T + 1) / 2 tiles and one square of T^2, one fp64 each, per subset
    assert query(1, 2) == 3 * 8 and query(3, 64) == 3 * 3 * 8 and query(3, 65) == 3 * (3 + 3 + 4) * 8
    assert query(100, 1000) == 100 * (136 + 136 + 256) * 8
    for S, m in ((0, 10), (-1, 10), (1, 1), (1, 0), (1, -5), (1 << 30, 4), (1 << 20, 1 << 12)):
        assert query(S, m) == 0, (S, m)


def test_new_entry_validates_without_a_device():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    P = 1 << 20           # never dereferenced: validation fails first
    bad, unsupported = _abi.IGAN_ERR_INVALID_ARGUMENT, _abi.IGAN_ERR_UNSUPPORTED

    def call(X=P, Y=P, idx_x=P, idx_y=P, partials=P, out=P, nx=8, ny=9, S=2, m=4, F=16):
        return lib.igan_poly3_kernel_sums(None, X, nx, Y, ny, idx_x, idx_y, S, m, F, 1.0 / 16, 1.0, partials, out)

    for b in ('X', 'Y', 'idx_x', 'idx_y', 'partials', 'out'):
        assert call(**{b: None}) == bad, b
        assert b'null buffer' in lib.igan_last_error()
    for F in (0, 4097, -1):
        assert call(F=F) == unsupported and b'1 <= F <= 4096' in lib.igan_last_error()
    for m in (1, 0, -2):
        assert call(m=m) == bad and b'm must be at least 2' in lib.igan_last_error()
    for S in (0, -1):
        assert call(S=S) == bad and b'S must be positive' in lib.igan_last_error()
    for n in ('nx', 'ny'):
        assert call(**{n: 0}) == bad and b'nx and ny' in lib.igan_last_error()
    assert call(S=1 << 30, m=4) == unsupported and b'31 bits' in lib.igan_last_error()
    assert call(X=P + 2) == bad and b'aligned' in lib.igan_last_error()
    assert call(out=P + 4) == bad and b'aligned' in lib.igan_last_error()
    with pytest.raises(ValueError):
        _abi.check(call(m=1))
    with pytest.raises(NotImplementedError):
        _abi.check(call(F=4097))


def test_binding_checks_indices_on_the_host():
    """An index equal to nx, a negative one, an F mismatch: ValueError before a device is touched (the tensors are host
    tensors here; a well-formed call then finds no device path)."""
    import torch
    from inclusivegan_amd import hip_ops
    X, Y = torch.zeros(5, 8), torch.zeros(7, 8)
    good = np.array([[0, 1, 2], [4, 3, 2]])
    for ix, iy in ((np.array([[0, 1, 5], [4, 3, 2]]), good), (good, np.array([[0, 1, 2], [7, 3, 2]])),
                   (np.array([[0, -1, 2], [4, 3, 2]]), good), (good, np.array([[0, 1, 2], [4, 3, -1]], np.int8))):
        with pytest.raises(ValueError, match='outside'):
            hip_ops.poly3_kernel_sums(X, Y, ix, iy, 0.125, 1.0)
    with pytest.raises(ValueError, match='one F'):
        hip_ops.poly3_kernel_sums(X, torch.zeros(7, 9), good, good, 0.125, 1.0)
    with pytest.raises(ValueError, match='one shape'):
        hip_ops.poly3_kernel_sums(X, Y, good, good[:1], 0.125, 1.0)
    with pytest.raises(ValueError, match='integer array'):
        hip_ops.poly3_kernel_sums(X, Y, good.astype(np.float64), good, 0.125, 1.0)
    with pytest.raises(TypeError, match='host'):
        hip_ops.poly3_kernel_sums(X, Y, torch.from_numpy(good), good, 0.125, 1.0)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.poly3_kernel_sums(X, Y, good, good.astype(np.uint16), 0.125, 1.0)


def test_kid_subsets_shapes_draws_and_clamps():
    k = KIDM()
    idx_fake, idx_real, m = k.kid_subsets(300, 260, 7, 100, 3)
    assert m == 100 and idx_fake.shape == idx_real.shape == (7, 100) and idx_fake.dtype == idx_real.dtype == np.int64
    for row in idx_fake:
        assert len(set(row.tolist())) == 100 and 0 <= row.min() and row.max() < 260
    for row in idx_real:
        assert len(set(row.tolist())) == 100 and 0 <= row.min() and row.max() < 300
    again = k.kid_subsets(300, 260, 7, 100, 3)
    assert np.array_equal(again[0], idx_fake) and np.array_equal(again[1], idx_real)
    assert not np.array_equal(k.kid_subsets(300, 260, 7, 100, 4)[0], idx_fake)
    # one RandomState(7): per subset first choice(num_fake = 9, 4), then choice(num_real = 11, 4); generated once with NumPy
    f, r, m = k.kid_subsets(11, 9, 2, 4, 7)
    assert m == 4 and f.tolist() == [[2, 7, 0, 8], [8, 5, 1, 0]] and r.tolist() == [[1, 2, 5, 3], [6, 1, 4, 2]]
    rnd = np.random.RandomState(7)
    assert [rnd.choice(9, 4, replace=False).tolist(), rnd.choice(11, 4, replace=False).tolist()] == [[2, 7, 0, 8], [1, 2, 5, 3]]
    # m clamps to the smaller set: a full draw is a permutation of it
    f, r, m = k.kid_subsets(40, 6, 3, 1000, 0)
    assert m == 6 and all(sorted(row.tolist()) == list(range(6)) for row in f) and r.max() < 40 and r.shape == (3, 6)
    f, r, m = k.kid_subsets(5, 60, 3, 1000, 0)
    assert m == 5 and all(sorted(row.tolist()) == list(range(5)) for row in r)
    for num_real, num_fake, cap in ((1, 50, 10), (50, 1, 10), (50, 50, 1), (0, 50, 10)):
        with pytest.raises(ValueError, match='m - 1'):
            k.kid_subsets(num_real, num_fake, 3, cap, 0)
    with pytest.raises(ValueError):
        k.kid_subsets(10, 10, 0, 5, 0)


def test_kid_from_sums_is_the_published_estimator():
    """An 8-row example: the NumPy fp64 restatement of the published code against kid_from_sums on the three sums of the same
    matrices, and against the oracle's exact evaluation."""
    rng = np.random.RandomState(5)
    m, F = 8, 16
    x = rng.randn(2, m, F).astype(np.float32)
    y = (rng.randn(2, m, F) + 1.5).astype(np.float32)
    sums, want_t = np.empty((2, 3)), np.empty(2)
    for s in range(2):
        xs, ys = x[s].astype(np.float64), y[s].astype(np.float64)
        kxx, kyy, kxy = (xs @ xs.T / F + 1) ** 3, (ys @ ys.T / F + 1) ** 3, (xs @ ys.T / F + 1) ** 3
        a, b = kxx + kyy, kxy
        want_t[s] = (a.sum() - np.diag(a).sum()) / (m - 1) - b.sum() * 2 / m
        sums[s] = [kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()]
    want = want_t.sum() / 2 / m
    kid, per_subset = KIDM().kid_from_sums(sums, m)
    assert isinstance(kid, float) and per_subset.shape == (2,) and per_subset.dtype == np.float64
    assert abs(kid) > 0.1                                    # nothing cancels in this example: 1e-12 relative is a statement
    assert abs(kid - want) <= 1e-12 * abs(want)
    assert np.all(np.abs(per_subset - want_t) <= 1e-12 * np.abs(want_t))
    exact = np.mean([kid_oracle.kid(x[s], y[s]) for s in range(2)])
    assert abs(kid - exact) <= 1e-12 * abs(exact)
    # one subset is its own mean; subsets are added in order
    assert KIDM().kid_from_sums(sums[:1], m)[0] == per_subset[0] / 1 / m
    assert KIDM().kid_from_sums(sums, m)[0] == (per_subset[0] + per_subset[1]) / 2 / m


def test_kid_from_sums_refuses_non_finite_sums():
    sums = np.ones((4, 3))
    sums[2, 1] = np.nan
    sums[3, 0] = np.inf
    with pytest.raises(FloatingPointError, match='subset 2 '):
        KIDM().kid_from_sums(sums, 5)
    with pytest.raises(ValueError):
        KIDM().kid_from_sums(np.ones((4, 2)), 5)
    with pytest.raises(ValueError):
        KIDM().kid_from_sums(np.ones((4, 3)), 1)


def test_oracle_budget_and_positions():
    """The oracle itself: sums against a plain double loop on a tiny case, a row listed twice counted as a pair, and the bound
    formula."""
    rng = np.random.RandomState(6)
    X, Y = rng.randn(6, 5).astype(np.float32), rng.randn(7, 5).astype(np.float32)
    ix, iy = np.array([[0, 3, 3, 5]]), np.array([[6, 1, 2, 4]])
    got, bound = kid_oracle.sums(X, Y, ix, iy, 0.2, 1.0)
    k = lambda a, b: (0.2 * float(np.dot(a.astype(np.float64), b.astype(np.float64))) + 1.0) ** 3
    x, y = X[ix[0]], Y[iy[0]]
    want = [sum(k(x[i], x[j]) for i in range(4) for j in range(4) if i != j), sum(k(y[i], y[j]) for i in range(4) for j in range(4) if i != j),
            sum(k(x[i], y[j]) for i in range(4) for j in range(4))]
    assert np.allclose(got[0], want, rtol=1e-13, atol=0)
    mags = kid_oracle.pair_magnitudes(x, y, 0.2, 1.0)
    assert np.all(mags >= np.abs(kid_oracle.pair_terms(x, y, 0.2, 1.0).astype(np.float64)))
    assert abs(bound[0, 2] / ((3 * 5 + 9 + 16) * 2.0 ** -53 * mags.sum()) - 1) < 1e-12                  # F = 5, 16 counted pairs
    mags = kid_oracle.pair_magnitudes(x, x, 0.2, 1.0)
    assert abs(bound[0, 0] / ((3 * 5 + 9 + 12) * 2.0 ** -53 * (mags.sum() - np.trace(mags))) - 1) < 1e-12   # 12 off the diagonal
    d, db = kid_oracle.diagonal_sums(X, ix, 0.2, 1.0)
    assert abs(d[0] - sum(k(a, a) for a in x)) <= 1e-12 * abs(d[0]) and db[0] > 0
    # positions 1 and 2 list row 3: the pair (1, 2) and (2, 1) are counted, each k(x_3, x_3)
    once = kid_oracle.sums(X, Y, np.array([[0, 3, 5]]), iy[:, :3], 0.2, 1.0)[0][0, 0]
    twice = got[0, 0]
    extra = 2 * k(X[3], X[3]) + 2 * (k(X[0], X[3]) + k(X[5], X[3]))
    assert abs((twice - once) - extra) <= 1e-12 * abs(extra)
