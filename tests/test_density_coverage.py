"""CPU: density and coverage (dc50k5) -- the parts that need no device.  The metric resolves from metric_defaults and takes an
injected feature network, the entry igan_ball_count_update in the header, the binding and its argument checks, and the closed
forms of the fp64 oracle (tests/dc_oracle.py) the GPU tests compare with."""
import ctypes
import os
import re

import numpy as np
import pytest

import dc_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dc50k5_resolves_to_the_dc_class():
    from inclusivegan_amd.metrics import density_coverage, metric_base
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    args = metric_defaults['dc50k5']
    assert args.func_name == 'metrics.density_coverage.DC'
    assert (args.num_images, args.nhood_size, args.minibatch_per_gpu, args.row_batch_size, args.col_batch_size) == (50000, 5, 8, 10000, 10000)
    m = metric_base.MetricGroup([args]).metrics[0]
    assert type(m) is density_coverage.DC and m.name == 'dc50k5'
    assert (m.num_images, m.nhood_size, m.row_batch_size, m.col_batch_size) == (50000, 5, 10000, 10000)
    assert density_coverage.DC.multi_rank is True
    assert '<=' in density_coverage.__doc__ and 'STRICT' in density_coverage.__doc__      # the difference from pr50k3 is stated


def test_dc_without_feature_fn_raises():
    from inclusivegan_amd.metrics import density_coverage
    m = density_coverage.DC(num_images=8, nhood_size=5, minibatch_per_gpu=4, row_batch_size=8, col_batch_size=8, name='dc8')
    with pytest.raises(RuntimeError, match='feature_fn'):
        m._evaluate(None, {}, 1)


def test_injected_feature_fn_reaches_the_metric():
    from inclusivegan_amd import run_metrics
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults

    def fn(images):
        return images

    args = run_metrics._with_injected(metric_defaults['dc50k5'], {'feature_fn': fn, 'classify_fn': fn})
    assert args.get('feature_fn') is fn and 'classify_fn' not in args
    assert 'feature_fn' not in metric_defaults['dc50k5']


def test_header_and_binding_of_the_new_entry():
    """The signature as the header states it: the stream, seven buffers and five ints, `inclusive` last."""
    from inclusivegan_amd import _abi
    header = open(os.path.join(ROOT, 'include', 'igan_hip.h')).read()
    m = re.search(r'\bint\s+igan_ball_count_update\s*\(([^;]*)\)\s*;', header)
    assert m is not None
    params = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')
    assert [p.split()[-1].lstrip('*') for p in params] == ['stream', 'query', 'qnorm', 'query_radius', 'cand', 'cnorm', 'count', 'dots',
                                                          'nq', 'nc', 'dim', 'nk', 'inclusive']
    assert 'long long* count' in m.group(1) and 'const double* query_radius' in m.group(1)
    lib = _abi.get_plugin()
    fn = lib.igan_ball_count_update
    assert len(fn.argtypes) == len(params) == 13
    assert list(fn.argtypes[-5:]) == [ctypes.c_int] * 5 and fn.restype is ctypes.c_int
    assert _abi.ABI_VERSION == 10 and lib.igan_abi_version() == 10
    assert re.search(r'#define\s+IGAN_ABI_VERSION\s+10\b', header)
    note = re.search(r'added under 10 without a bump.*?\*/', header, flags=re.S).group(0)
    assert 'igan_ball_count_update' in note


def test_new_entry_validates_without_a_device():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    P = 1 << 20           # never dereferenced: validation fails first
    bad = _abi.IGAN_ERR_INVALID_ARGUMENT

    def count(query=P, qnorm=P, radii=P, cand=P, cnorm=P, counts=P, dots=P, nq=4, nc=64, dim=16, nk=1, inclusive=0):
        return lib.igan_ball_count_update(None, query, qnorm, radii, cand, cnorm, counts, dots, nq, nc, dim, nk, inclusive)

    for b in ('query', 'qnorm', 'radii', 'cand', 'cnorm', 'counts', 'dots'):
        assert count(**{b: None}) == bad, b
        assert b'null buffer' in lib.igan_last_error()
    for size in ('nq', 'nc', 'dim'):
        for v in (0, -3):
            assert count(**{size: v}) == bad, size
            assert b'sizes must be positive' in lib.igan_last_error()
    assert count(nq=1 << 20, dim=1 << 10) == bad and b'2 GiB' in lib.igan_last_error()
    assert count(nc=1 << 20, dim=1 << 10) == bad and b'2 GiB' in lib.igan_last_error()
    assert count(nq=1 << 16, nc=1 << 16, dim=4) == bad and b'too large' in lib.igan_last_error()
    for nk in (0, 9, -1):
        assert count(nk=nk) == bad and b'nk' in lib.igan_last_error()
    for inclusive in (2, -1):
        assert count(inclusive=inclusive) == bad and b'inclusive' in lib.igan_last_error()
    with pytest.raises(ValueError):
        _abi.check(count(inclusive=2))


def test_python_layer_has_no_cpu_path():
    import torch
    from inclusivegan_amd import hip_ops
    for nk in (0, 9):
        with pytest.raises(ValueError):
            hip_ops.ball_count_state(4, nk, 'cpu')
    state = hip_ops.ball_count_state(4, 3, 'cpu')
    assert state.shape == (4, 3) and state.dtype == torch.int64 and int(state.abs().sum()) == 0
    q = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.ball_count_update_raw(q, torch.zeros(4), torch.zeros(4, 3, dtype=torch.float64), q, torch.zeros(4), state)


@pytest.mark.parametrize('k', [1, 3, 5])
def test_oracle_of_a_set_against_itself(k):
    """Distinct distances: the ball of a point holds, strictly, itself and its k - 1 nearest -- k points; the k-th neighbour
    sits on the sphere and joins when the comparison is inclusive."""
    x = np.random.RandomState(3).randn(97, 24).astype(np.float32)
    d2 = dc_oracle.exact_sqdist(x, x)
    assert all(len(np.unique(row)) == row.size for row in d2)
    got = dc_oracle.density_coverage(x, x, [k])
    assert np.array_equal(got['counts'], np.full((97, 1), k))
    assert got['density'] == [1.0] and got['coverage'] == [1.0]
    inc = dc_oracle.density_coverage(x, x, [k], inclusive=True)
    assert np.array_equal(inc['counts'], np.full((97, 1), k + 1))
    assert inc['density'] == [(k + 1) / k] and inc['coverage'] == [1.0]
    assert dc_oracle.exact_ties(d2, got['radii']) == 97


def test_oracle_refuses_an_undecided_case():
    """A fake a hair inside a sphere (relative gap 1e-12) is neither clear of the radius nor an exact tie."""
    x = np.random.RandomState(4).randn(12, 6)
    x = (np.round(x * 64) / 64).astype(np.float32)        # few mantissa bits: room for an exactly representable nudge
    r2 = dc_oracle.radii(x, [2])
    fakes = x.copy()
    assert not dc_oracle.undecided(dc_oracle.exact_sqdist(x, fakes), r2, x, fakes)
    d2 = dc_oracle.exact_sqdist(x, fakes)
    i, j = 0, int(np.argsort(d2[0], kind='stable')[2])
    d2[i, j] *= 1.0 - 1e-12
    assert dc_oracle.undecided(d2, r2, x, fakes) == [(i, j, 0)]
    with pytest.raises(AssertionError, match='undecided'):
        dc_oracle.assert_decided(d2, r2, x, fakes)
