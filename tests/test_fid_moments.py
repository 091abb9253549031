"""CPU: the streaming-moments entry points behind FID (csrc/moments.hip) validate their arguments before a device is touched,
the Python layer has no CPU path, and MetricBase names the cache file of real statistics as the reference does
(metrics/metric_base.py:110-117), with the injected feature network added to the hash."""
import hashlib
import os

import numpy as np
import pytest
import torch


def named_feature_fn(images):
    return images


def other_feature_fn(images):
    return images


def test_entry_points_validate_without_a_device():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    assert lib.igan_abi_version() == _abi.ABI_VERSION == 10          # new exports only: no bump
    P = 1 << 20           # never dereferenced: validation fails first
    bad, unsupported = _abi.IGAN_ERR_INVALID_ARGUMENT, _abi.IGAN_ERR_UNSUPPORTED

    def update(n=100, F=64, **null):
        X, shift, s, g = (None if b in null else P for b in ('X', 'shift', 'sum', 'gram'))
        return lib.igan_moments_update(None, X, shift, s, g, None, 0, n, F)

    def finalize(n_total=100, F=64, **null):
        s, g, shift, mean, cov = (None if b in null else P * (i + 1) for i, b in enumerate(('sum', 'gram', 'shift', 'mean', 'cov')))
        return lib.igan_moments_finalize(None, s, g, shift, mean, cov, n_total, F)

    for F in (0, 4097, -1):
        assert update(F=F) == unsupported and b'F <= 4096' in lib.igan_last_error()
        assert finalize(F=F) == unsupported and b'F <= 4096' in lib.igan_last_error()
    for n in (0, -3):
        assert update(n=n) == bad and b'n must be positive' in lib.igan_last_error()
    for b in ('X', 'sum', 'gram'):
        assert update(**{b: None}) == bad and b'null buffer' in lib.igan_last_error(), b
    for b in ('sum', 'gram', 'mean', 'cov'):
        assert finalize(**{b: None}) == bad and b'null buffer' in lib.igan_last_error(), b
    assert update(n=1 << 19, F=1 << 10) == bad and b'2 GiB' in lib.igan_last_error()           # n * F * 4 == 2 GiB exactly
    assert update(n=(1 << 17) + 1, F=4096) == bad and b'2 GiB' in lib.igan_last_error()
    for n_total in (1, 0, -7):
        assert finalize(n_total=n_total) == bad and b'at least 2' in lib.igan_last_error()
    with pytest.raises(NotImplementedError):
        _abi.check(update(F=4097))
    with pytest.raises(ValueError):
        _abi.check(finalize(n_total=1))
    ws = lib.igan_moments_workspace_bytes
    assert ws(2048, 2048) == ws(2048, 2048) and ws(1, 1) % 16 == 0 and ws(8, 4096) % 16 == 0      # a function of the sizes alone


def test_python_layer_has_no_cpu_path():
    from inclusivegan_amd import hip_ops
    x = torch.zeros(8, 4)
    s, g = torch.zeros(4, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.moments_update_raw(x, None, s, g)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.moments_finalize_raw(s, g, None, 8)
    with pytest.raises(NotImplementedError):
        hip_ops.FeatureMoments(4097, 'cpu')
    with pytest.raises(NotImplementedError):
        hip_ops.FeatureMoments(0, 'cpu')
    assert 1 <= hip_ops.MOMENTS_CHUNK_ROWS and hip_ops.MOMENTS_CHUNK_ROWS * hip_ops.MOMENTS_MAX_F * 4 < 2 ** 31


def _metric(feature_fn=None, **run):
    from inclusivegan_amd.metrics import frechet_inception_distance as F
    m = F.FID(num_images=50000, minibatch_per_gpu=8, feature_fn=feature_fn, name='fid50k')
    m._configure('snapshot.pkl', **run)
    return m


def test_cache_file_for_reals_is_the_references_name():
    dataset_args = dict(tfrecord_dir='datasets/celeba_30k', max_label_size=0, resolution=128, shuffle_mb=0)
    m = _metric(data_dir='data', dataset_args=dataset_args, mirror_augment=True)

    def reference(name, mirror_augment, dataset_args, extension='pkl', **kwargs):        # metric_base.py:110-117, restated
        all_args = dict(metric_name=name, mirror_augment=mirror_augment)
        all_args.update(dataset_args)
        all_args.update(kwargs)
        md5 = hashlib.md5(repr(sorted(all_args.items())).encode('utf-8'))
        dataset_name = os.path.splitext(os.path.basename(dataset_args.get('tfrecord_dir', None)))[0]
        return os.path.join('.stylegan2-cache', '%s-%s-%s.%s' % (md5.hexdigest(), name, dataset_name, extension))

    assert m._get_cache_file_for_reals(num_images=50000) == reference('fid50k', True, dataset_args, num_images=50000)
    assert m._get_cache_file_for_reals(extension='npz', num_images=7, x='y') == reference('fid50k', True, dataset_args, extension='npz', num_images=7, x='y')
    assert os.path.basename(m._get_cache_file_for_reals()).endswith('-fid50k-celeba_30k.pkl')
    # the injected network is part of the hash, by module and qualified name
    a = m._get_cache_file_for_reals(feature_fn=named_feature_fn, num_images=50000)
    b = m._get_cache_file_for_reals(feature_fn=other_feature_fn, num_images=50000)
    assert a != b and a != m._get_cache_file_for_reals(num_images=50000)
    assert a == reference('fid50k', True, dataset_args, num_images=50000, feature_fn=__name__ + '.named_feature_fn')
    assert a == m._get_cache_file_for_reals(feature_fn=named_feature_fn, num_images=50000)
    assert a != m._get_cache_file_for_reals(feature_fn=named_feature_fn, num_images=49999)
    m2 = _metric(data_dir='data', dataset_args=dataset_args, mirror_augment=False)
    assert m2._get_cache_file_for_reals(feature_fn=named_feature_fn, num_images=50000) != a


def test_cache_file_for_reals_is_none_without_a_name():
    def local_fn(images):
        return images

    class Net:
        def __call__(self, images):
            return images

    tfr = dict(tfrecord_dir='celeba_30k', resolution=128)
    m = _metric(data_dir='data', dataset_args=tfr, mirror_augment=False)
    assert m._get_cache_file_for_reals(feature_fn=named_feature_fn) is not None
    assert m._get_cache_file_for_reals(feature_fn=lambda images: images) is None
    assert m._get_cache_file_for_reals(feature_fn=local_fn) is None
    assert m._get_cache_file_for_reals(feature_fn=Net()) is None
    synthetic = _metric(data_dir=None, dataset_args=dict(resolution=32, num_channels=3, label_size=0, data_size=128), mirror_augment=False)
    assert synthetic._get_cache_file_for_reals(feature_fn=named_feature_fn, num_images=96) is None
    assert _metric()._get_cache_file_for_reals(feature_fn=named_feature_fn) is None          # no dataset args at all


def test_host_features_take_the_host_path():
    """NumPy features never touch the device path: FID._statistics on host arrays is np.mean / np.cov, and a non-finite
    feature raises instead of reaching sqrtm."""
    from inclusivegan_amd.metrics import frechet_inception_distance as F
    rng = np.random.RandomState(3)
    act = rng.randn(40, 6).astype(np.float32)
    m = F.FID(num_images=40, minibatch_per_gpu=16, feature_fn=named_feature_fn, name='fid40')
    mu, sigma = m._statistics(iter([act[:16], torch.from_numpy(act[16:32]), act[32:]]), 'real')
    want_mu, want_sigma = F.statistics(act)
    assert np.array_equal(mu, want_mu) and np.array_equal(sigma, want_sigma)
    act[17, 2] = np.nan
    act[3, 4] = np.inf
    with pytest.raises(FloatingPointError, match='2 of the 6 columns'):
        m._statistics(iter([act]), 'fake')
