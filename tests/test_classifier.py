"""CPU: the host-side pieces of the Stacked-MNIST mode classifier -- argument validation of the three softmax cross-entropy
entry points before a device is touched, the digit <-> number place values, joint_logits against fp64, and the metric classes'
rules for where the classifier comes from (an injected function wins; no function and no pickle is the old error)."""
import ctypes
import os

import numpy as np
import pytest
import torch


def test_xent_entry_points_reject_invalid_arguments_without_a_device():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    INV = _abi.IGAN_ERR_INVALID_ARGUMENT
    p = ctypes.c_void_p(64)           # never dereferenced: validation fails first
    odd = ctypes.c_void_p(68)         # 4-byte aligned only

    def err():
        return lib.igan_last_error()

    fwd = lambda **o: lib.igan_softmax_xent_fwd(None, o.get('x', p), o.get('lab', p), o.get('loss', p), o.get('lse', p), o.get('pred', p), o.get('n', 4), o.get('K', 10))
    bwd = lambda **o: lib.igan_softmax_xent_bwd(None, o.get('x', p), o.get('lab', p), o.get('lse', p), o.get('dloss', p), o.get('dx', p), o.get('n', 4), o.get('K', 10))
    sta = lambda **o: lib.igan_xent_stats_update(None, o.get('loss', p), o.get('lab', p), o.get('pred', p), o.get('sum', p), o.get('counts', p), o.get('n', 4), o.get('K', 10))
    for call, name, nullable in ((fwd, b'softmax_xent_fwd', ('x', 'lab', 'loss', 'lse')), (bwd, b'softmax_xent_bwd', ('x', 'lab', 'lse', 'dloss', 'dx')),
                                 (sta, b'xent_stats_update', ('loss', 'lab', 'pred', 'sum', 'counts'))):
        for arg in nullable:
            assert call(**{arg: None}) == INV and err() == name + b': null buffer', (name, arg)
        assert call(n=0) == INV and err() == name + b': n must be positive'
        assert call(K=0) == INV and err() == name + b': K must be positive'
        assert call(n=-3) == INV and call(K=-1) == INV
        assert call(n=1 << 19, K=1 << 10) == INV and b'2 GiB' in err()              # n * K * 4 == 2 GiB exactly
        assert call(n=1 << 30, K=1 << 30) == INV and b'2 GiB' in err()              # the product is taken in 64 bits
    assert fwd(lse=odd) == INV and err() == b'softmax_xent_fwd: lse must be 8-byte aligned'
    assert bwd(lse=odd) == INV and err() == b'softmax_xent_bwd: lse must be 8-byte aligned'
    assert sta(sum=odd) == INV and err() == b'xent_stats_update: loss_sum / counts must be 8-byte aligned'
    assert sta(counts=odd) == INV and err() == b'xent_stats_update: loss_sum / counts must be 8-byte aligned'
    assert fwd(x=ctypes.c_void_p(66)) == INV and b'4-byte aligned' in err()
    with pytest.raises(ValueError, match='lse must be 8-byte aligned'):
        _abi.check(fwd(lse=odd))


def test_digits_and_numbers_round_trip_with_the_data_set_tools_place_values():
    import inspect
    from inclusivegan_amd import dataset_tool
    from inclusivegan_amd.training import networks_classifier as NC
    numbers = np.arange(1000)
    digits = NC.digits_of_number(numbers)
    assert digits.shape == (1000, 3) and digits.min() == 0 and digits.max() == 9
    assert np.array_equal(NC.number_of_digits(digits), numbers)
    assert len({tuple(d) for d in digits}) == 1000
    # create_mnistrgb: number = dot(digit labels of the (R, G, B) planes, [1, 10, 100])
    assert 'place_value = np.array([1, 10, 100])' in inspect.getsource(dataset_tool.create_mnistrgb)
    assert tuple(NC.PLACE_VALUES) == (1, 10, 100)
    assert np.array_equal(digits @ np.array([1, 10, 100]), numbers)
    assert tuple(NC.digits_of_number(907)) == (7, 0, 9)
    from inclusivegan_amd.train_classifier import class_targets
    onehot = np.zeros((2, 1000), np.float32)
    onehot[0, 907] = onehot[1, 45] = 1
    assert class_targets(onehot, 'digits').tolist() == [7, 0, 9, 5, 4, 0] and class_targets(onehot, 'onehot').tolist() == [907, 45]


def test_joint_logits_against_fp64():
    from inclusivegan_amd.training import networks_classifier as NC
    rng = np.random.RandomState(3)
    n = 64
    x = rng.randint(-6, 7, size=(n, 3, 10)).astype(np.float32)
    top = rng.randint(10, size=(n, 3))
    x[np.arange(n)[:, None], np.arange(3)[None, :], top] = 9.0          # integer-valued, a unique maximum per channel
    got = NC.joint_logits(torch.from_numpy(x))
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 1000)
    got = got.numpy()
    assert np.array_equal(np.argmax(got, axis=1), NC.number_of_digits(top))
    x64 = x.astype(np.float64)
    ls = x64 - (np.max(x64, axis=2, keepdims=True) + np.log(np.sum(np.exp(x64 - np.max(x64, axis=2, keepdims=True)), axis=2, keepdims=True)))
    d = NC.digits_of_number(np.arange(1000))                             # [1000, 3]
    terms = np.stack([ls[:, c, d[:, c]] for c in range(3)], axis=0)      # [3, n, 1000]
    want = terms.sum(axis=0)
    bound = 4 * 2.0 ** -24 * np.abs(terms).sum(axis=0)
    err = np.abs(got.astype(np.float64) - want)
    print('joint_logits: worst error / bound %.3f' % float(np.max(err / bound)))
    assert np.all(err <= bound)


def _metric(cls_name, **kw):
    from inclusivegan_amd.metrics import KL, mode_counts
    cls = dict(mode_counts=mode_counts.mode_counts, KL=KL.KL)[cls_name]
    return cls(num_images=4, minibatch_per_gpu=2, name=cls_name + '_tiny', **kw)


@pytest.mark.parametrize('cls_name', ['mode_counts', 'KL'])
def test_metrics_without_classifier_raise_the_old_error(cls_name, tmp_path, monkeypatch):
    from inclusivegan_amd.metrics import mode_counts as MC
    monkeypatch.chdir(tmp_path)                                         # no metrics/stacked_mnist_classifier.pkl here
    m = _metric(cls_name)
    assert m.classifier_pkl == 'metrics/stacked_mnist_classifier.pkl' and m.classify_fn is None
    old = "%s needs classify_fn: the reference's metrics/stacked_mnist_classifier.pkl is not available in this tree" % m.name
    for fn, args in ((MC.class_statistics, (m, None, {}, 1)), (MC.predicted_labels, (m, None, {}, 1)), (MC.shard_histogram, (m, None, {}, 0, 1))):
        with pytest.raises(RuntimeError) as e:
            fn(*args)
        assert str(e.value).startswith(old) and 'train_classifier' in str(e.value)
    with pytest.raises(RuntimeError, match='needs classify_fn'):
        MC.class_statistics(_metric(cls_name, classifier_pkl=str(tmp_path / 'absent.pkl')), None, {}, 1)


@pytest.mark.parametrize('cls_name', ['mode_counts', 'KL'])
def test_an_injected_function_wins_over_a_pickle(cls_name, tmp_path):
    from inclusivegan_amd.metrics import mode_counts as MC
    pkl = tmp_path / 'classifier.pkl'
    pkl.write_bytes(b'not a pickle: opening it would fail')
    calls = []

    def classify(images):
        calls.append(images.shape[0])
        return np.eye(5, dtype=np.float32)[[1, 3]]

    m = _metric(cls_name, classify_fn=classify, classifier_pkl=str(pkl))
    m._generate = lambda Gs, mb, kw, as_uint8: np.zeros((mb, 3, 4, 4), np.float32)
    counts, labels_all, K = MC.class_statistics(m, None, {}, 1)
    assert m.classify_fn is classify and calls == [2, 2] and K == 5
    assert counts is None and labels_all.tolist() == [1, 3, 1, 3]
