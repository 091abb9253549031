"""CPU: perceptual path length (ppl_zfull .. ppl2_wend).  The table entries carry the reference's arguments and resolve to PPL;
the crop geometry and the outlier filter equal their closed forms; the two HIP entry points validate their arguments before
anything touches a device; the Python layer has no CPU path."""
import math

import numpy as np
import pytest

REFERENCE_TABLE = {        # metrics/metric_defaults.py:20-24
    'ppl_zfull': ('z', 'full', True),
    'ppl_wfull': ('w', 'full', True),
    'ppl_zend': ('z', 'end', True),
    'ppl_wend': ('w', 'end', True),
    'ppl2_wend': ('w', 'end', False),
}


def test_table_entries_carry_the_reference_values_and_resolve_to_ppl():
    from inclusivegan_amd.metrics import metric_base, perceptual_path_length
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    for name, (space, sampling, crop) in REFERENCE_TABLE.items():
        args = metric_defaults[name]
        assert args.func_name == 'metrics.perceptual_path_length.PPL'
        assert dict(args) == dict(name=name, func_name='metrics.perceptual_path_length.PPL', num_samples=50000, epsilon=1e-4, space=space,
                                  sampling=sampling, crop=crop, minibatch_per_gpu=4, Gs_overrides=dict(dtype='float32', mapping_dtype='float32'))
        m = metric_base.MetricGroup([args]).metrics[0]
        assert type(m) is perceptual_path_length.PPL and m.name == name
        assert (m.num_samples, m.epsilon, m.space, m.sampling, m.crop, m.minibatch_per_gpu) == (50000, 1e-4, space, sampling, crop, 4)
        assert m.Gs_overrides == dict(dtype='float32', mapping_dtype='float32')
    for name in ('normalize', 'slerp', 'PPL', 'crop_geometry', 'reject_outliers'):
        assert hasattr(perceptual_path_length, name)


def test_bad_space_and_sampling_raise():
    from inclusivegan_amd.metrics.perceptual_path_length import PPL
    kw = dict(num_samples=8, epsilon=1e-4, crop=True, minibatch_per_gpu=4, Gs_overrides={}, name='ppl')
    with pytest.raises(AssertionError):
        PPL(space='x', sampling='full', **kw)
    with pytest.raises(AssertionError):
        PPL(space='w', sampling='mid', **kw)
    assert PPL(space='w', sampling='end', **kw).name == 'ppl'


def test_crop_geometry():
    from inclusivegan_amd.metrics.perceptual_path_length import crop_geometry
    assert crop_geometry(128, 128, True) == (48, 112, 32, 96, 1)
    assert crop_geometry(1024, 1024, True) == (384, 896, 256, 768, 2)
    assert crop_geometry(1024, 1024, False) == (0, 1024, 0, 1024, 4)
    assert crop_geometry(32, 32, True) == (12, 28, 8, 24, 1)
    assert crop_geometry(256, 256, False) == (0, 256, 0, 256, 1)        # 256 // 256 == 1: nothing to do
    assert crop_geometry(512, 512, True) == (192, 448, 128, 384, 1)     # the factor is taken after the crop


def closed_form_filter(d):
    s = np.sort(d)
    n = len(s)
    lo, hi = s[int(math.floor(0.01 * (n - 1)))], s[int(math.ceil(0.99 * (n - 1)))]
    return d[(lo <= d) & (d <= hi)]


@pytest.mark.parametrize('case', ['n100', 'n101', 'ties', 'n1'])
def test_reject_outliers_equals_the_closed_form(case):
    from inclusivegan_amd.metrics.perceptual_path_length import reject_outliers
    rng = np.random.RandomState(7)
    if case == 'n100':
        d = rng.rand(100).astype(np.float32)
    elif case == 'n101':
        d = rng.rand(101).astype(np.float32)
    elif case == 'ties':
        d = rng.rand(300).astype(np.float32)
        s = np.sort(d)
        d[d <= s[4]] = s[2]             # five values share the lower bound (position floor(2.99) = 2)
        d[d >= s[-5]] = s[-3]           # five share the upper bound (position ceil(296.01) = 297)
    else:
        d = np.array([3.5], np.float32)
    got = reject_outliers(d)
    want = closed_form_filter(d)
    assert np.array_equal(got, want) and got.dtype == d.dtype
    if case == 'n100':
        assert len(got) == 100              # floor(.99) = 0 and ceil(98.01) = 99: the bounds are the minimum and the maximum
    if case == 'n101':
        assert len(got) == 99 and d.min() not in got and d.max() not in got     # floor(1.0) = 1 and ceil(99.0) = 99 of 0 .. 100
    if case == 'ties':
        assert (got == np.sort(d)[2]).sum() == 5 and (got == np.sort(d)[297]).sum() == 5    # both bounds are inclusive
    if case == 'n1':
        assert got.tolist() == [3.5]


def test_entry_points_validate_without_a_device():
    from inclusivegan_amd import _abi
    assert _abi.ABI_VERSION == 10
    lib = _abi.get_plugin()
    assert lib.igan_abi_version() == 10
    assert 'igan_ppl_endpoints' in _abi.SIGNATURES and 'igan_ppl_crop_prep' in _abi.SIGNATURES
    assert hasattr(lib, 'igan_ppl_endpoints') and hasattr(lib, 'igan_ppl_crop_prep')
    P, Q = 1 << 20, 1 << 24           # never dereferenced: validation fails first
    bad = _abi.IGAN_ERR_INVALID_ARGUMENT

    def endpoints(lat=P, t=P + 4096, out=Q, n=4, dim=512, epsilon=1e-4, mode=0):
        return lib.igan_ppl_endpoints(None, lat, t, out, n, dim, epsilon, mode)

    def crop(x=P, y=Q, N=2, C=3, H=32, W=32, y0=12, y1=28, x0=8, x1=24, factor=1, strides=(3072, 1, 96, 3)):
        return lib.igan_ppl_crop_prep(None, x, y, N, C, H, W, y0, y1, x0, x1, factor, *strides)

    def rejected(rc, text):
        return rc == bad and text in lib.igan_last_error()

    for b in ('lat', 't', 'out'):
        assert rejected(endpoints(**{b: None}), b'null buffer'), b
    for size in ('n', 'dim'):
        for v in (0, -3):
            assert rejected(endpoints(**{size: v}), b'sizes must be positive'), size
    assert rejected(endpoints(n=1 << 20, dim=1 << 11), b'too large')
    for mode in (-1, 2, 7):
        assert rejected(endpoints(mode=mode), b'mode')
    for eps in (float('nan'), float('inf'), -float('inf')):
        assert rejected(endpoints(epsilon=eps), b'epsilon')
    assert rejected(endpoints(out=P), b'alias')
    assert rejected(endpoints(out=P + 4 * (2 * 4 * 512 - 1)), b'alias')          # the last value of lat
    assert rejected(endpoints(lat=Q + 4 * (2 * 4 * 512 - 1)), b'alias')          # the last value of out

    for b in ('x', 'y'):
        assert rejected(crop(**{b: None}), b'null buffer'), b
    assert rejected(crop(y=Q + 4), b'16-byte')
    for size in ('N', 'C', 'H', 'W'):
        for v in (0, -1):
            assert rejected(crop(**{size: v}), b'sizes must be positive'), size
    for window in (dict(y0=-1), dict(y1=33), dict(x0=-2), dict(x1=40), dict(y0=28, y1=28), dict(x0=24, x1=8)):
        assert rejected(crop(**window), b'window'), window
    for factor in (0, -2):
        assert rejected(crop(factor=factor), b'factor must be >= 1')
    for factor in (3, 5, 32):
        assert rejected(crop(factor=factor), b'divide'), factor
    assert rejected(crop(x0=8, x1=22, factor=4), b'divide')                      # 16 rows divide, 14 columns do not
    assert rejected(crop(strides=(3072, 1, -96, 3)), b'strides')
    with pytest.raises(ValueError, match='mode'):
        _abi.check(endpoints(mode=2))


def test_python_layer_has_no_cpu_path():
    import torch
    from inclusivegan_amd import hip_ops
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.ppl_endpoints_raw(torch.zeros(4, 8), torch.zeros(2), 1e-4, 0)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.ppl_crop_prep_raw(torch.zeros(2, 3, 16, 16), (0, 16, 0, 16), 1)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.lpips_adjacent_pairs_raw([torch.zeros(4, 64, 2, 2)], [torch.zeros(64)])
