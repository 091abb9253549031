"""CPU: the host-side pieces of the CelebA attribute classifier -- the four sigmoid cross-entropy entry points are exported,
bound and validate before a device is touched, the Python layer has no CPU path, the fp64 oracle of tests/bce_oracle.py has the
properties the kernels are tested against, linear separability's attribute order maps onto the data set's columns, and the
rules for where `ls` takes its classifier from (injected functions win; none and no pickle is the old error)."""
import ctypes

import numpy as np
import pytest
import torch

import bce_oracle as O

NAMES = ('igan_sigmoid_xent_fwd', 'igan_sigmoid_xent_bwd', 'igan_sigmoid_xent_stats_update', 'igan_binary_probs')


def test_entry_points_are_exported_and_bound_at_abi_10():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    for name in NAMES:
        assert name in _abi.SIGNATURES and hasattr(lib, name), name
    assert _abi.ABI_VERSION == 10 and lib.igan_abi_version() == 10


def test_entry_points_reject_invalid_arguments_without_a_device():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    INV = _abi.IGAN_ERR_INVALID_ARGUMENT
    p = ctypes.c_void_p(64)           # never dereferenced: validation fails first
    odd = ctypes.c_void_p(68)         # 4-byte aligned only

    def err():
        return lib.igan_last_error()

    fwd = lambda **o: lib.igan_sigmoid_xent_fwd(None, o.get('x', p), o.get('t', p), o.get('w', p), o.get('loss', p), o.get('pred', p), o.get('n', 4), o.get('A', 40))
    bwd = lambda **o: lib.igan_sigmoid_xent_bwd(None, o.get('x', p), o.get('t', p), o.get('w', p), o.get('dloss', p), o.get('dx', p), o.get('n', 4), o.get('A', 40))
    sta = lambda **o: lib.igan_sigmoid_xent_stats_update(None, o.get('loss', p), o.get('x', p), o.get('t', p), o.get('sum', p), o.get('counts', p), o.get('n', 4), o.get('A', 40))
    prb = lambda **o: lib.igan_binary_probs(None, o.get('x', p), o.get('probs', p), o.get('n', 4), o.get('A', 40))
    for call, name, required in ((fwd, b'sigmoid_xent_fwd', ('x', 't', 'loss')), (bwd, b'sigmoid_xent_bwd', ('x', 't', 'dloss', 'dx')),
                                 (sta, b'sigmoid_xent_stats_update', ('loss', 'x', 't', 'sum', 'counts')), (prb, b'binary_probs', ('x', 'probs'))):
        for arg in required:
            assert call(**{arg: None}) == INV and err() == name + b': null buffer', (name, arg)
        assert call(n=0) == INV and err() == name + b': n must be positive'
        assert call(A=0) == INV and err() == name + b': A must be positive'
        assert call(n=-3) == INV and call(A=-1) == INV
        assert call(n=1 << 19, A=1 << 10) == INV and b'2 GiB' in err()              # n * A * 4 == 2 GiB exactly
        assert call(n=1 << 30, A=1 << 30) == INV and b'2 GiB' in err()              # the product is taken in 64 bits
        assert call(x=ctypes.c_void_p(66)) == INV and b'4-byte aligned' in err()
    assert sta(sum=odd) == INV and err() == b'sigmoid_xent_stats_update: loss_sum / counts must be 8-byte aligned'
    assert sta(counts=odd) == INV and err() == b'sigmoid_xent_stats_update: loss_sum / counts must be 8-byte aligned'
    assert prb(probs=odd) == INV and err() == b'binary_probs: probs must be 8-byte aligned'
    assert fwd(w=ctypes.c_void_p(66)) == INV and b'4-byte aligned' in err()
    with pytest.raises(ValueError, match='A must be positive'):
        _abi.check(fwd(A=0))


def test_python_layer_has_no_cpu_path():
    from inclusivegan_amd import hip_ops
    x, t = torch.zeros(2, 3), torch.zeros(2, 3)
    calls = (lambda: hip_ops.sigmoid_xent_raw(x, t), lambda: hip_ops.sigmoid_xent_bwd_raw(x, t, x), lambda: hip_ops.binary_probs(x),
             lambda: hip_ops.SigmoidXentFn.apply(x, t),
             lambda: hip_ops.sigmoid_xent_stats_update_raw(x, x, t, torch.zeros(3, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.int64)))
    for call in calls:
        with pytest.raises(RuntimeError, match='no CPU path'):
            call()
    with pytest.raises(ValueError, match='A must be positive'):
        hip_ops.BinaryXentStats(0, 'cpu')


def test_oracle_properties():
    x32 = np.concatenate([O.logits_of(257, 40, seed=1).reshape(-1), np.linspace(-40, 40, 321).astype(np.float32)])
    x32 = x32[np.abs(x32) < 1e4]
    # softplus(x) - softplus(-x) == x, to the rounding of the two values in fp64
    x = x32.astype(np.float64)
    sp, sm = O.softplus(x), O.softplus(-x)
    assert np.all(np.abs((sp - sm) - x) <= 2 * np.spacing(np.maximum(sp, sm)))
    assert np.isnan(O.softplus(np.array([np.nan]))[0]) and O.softplus(np.array([-np.inf]))[0] == 0 and O.softplus(np.array([np.inf]))[0] == np.inf
    # the gradients are the derivative of the loss: central differences in np.longdouble at moderate logits
    xm = x32[np.abs(x32) < 30].reshape(-1, 1)
    xm = xm[:xm.shape[0] // 4 * 4].reshape(-1, 4)
    w = np.array([1.0, 0.25, 3.5, 2.0], np.float32)
    h = np.longdouble(2.0) ** -20
    for tval in (0.0, 1.0):
        t = np.full(xm.shape, tval, np.float32)
        z = xm.astype(np.longdouble)
        loss_at = lambda zz: np.where(tval == 1.0, w.astype(np.longdouble)[None, :] * O.softplus(-zz), O.softplus(zz))
        numeric = (loss_at(z + h) - loss_at(z - h)) / (2 * h)
        analytic = O.backward(xm, t, np.ones_like(xm), w)
        # the central difference is off by h^2 / 6 |f'''| <= h^2 w / 36 and by the rounding of the loss values, 2^-63 |f| / h
        tol = (h * h * 4 + np.longdouble(2.0) ** -62 * np.abs(loss_at(z)) / h).astype(np.float64)
        assert np.all(np.abs((numeric - analytic).astype(np.float64)) <= tol)
    # ignored targets: no loss, no gradient
    t = np.array([[np.nan, -1.0, 0.5, 2.0]], np.float32)
    xi = np.array([[3.0, -2.0, np.nan, np.inf]], np.float32)
    assert not np.any(O.forward(xi, t)[0]) and not np.any(O.backward(xi, t, np.ones_like(xi)))
    # +inf: loss 0 at a positive, +inf at a negative; a NaN logit is a NaN loss and predicts 0
    loss, pred = O.forward(np.array([[np.inf, np.inf, np.nan]], np.float32), np.array([[1.0, 0.0, 1.0]], np.float32))
    assert loss[0, 0] == 0 and loss[0, 1] == np.inf and np.isnan(loss[0, 2]) and pred.tolist() == [[1, 1, 0]]
    # p0 + p1 == 1 to rounding, attribute-major, with the factor 2
    probs = O.binary_probs(x32.reshape(-1, 1), dtype=np.float64)
    assert probs.shape == (1, x32.size, 2) and np.all(np.abs(probs.sum(axis=2) - 1.0) <= 2.0 ** -52)
    assert abs(O.binary_probs(np.array([[0.5]], np.float32), dtype=np.float64)[0, 0, 0] - 1 / (1 + np.exp(-1.0))) <= 2.0 ** -52
    both = O.binary_probs(np.arange(6, dtype=np.float32).reshape(2, 3), dtype=np.float64)
    assert both.shape == (3, 2, 2) and both[2, 1, 0] == 1 / (1 + np.exp(-10.0))


def test_ls_attribute_order_maps_onto_the_data_sets_columns():
    from inclusivegan_amd.metrics import linear_separability as ls
    from inclusivegan_amd.training.imle import CELEBA_ATTRIBUTES
    names = ls.LS_ATTRIBUTE_NAMES
    assert len(names) == 40 and sorted(names) == sorted(CELEBA_ATTRIBUTES)
    assert names[0] == 'Male' and names[19] == 'Eyeglasses' and names[39] == 'Wearing_Necktie'
    assert names[:5] == ('Male', 'Smiling', 'Attractive', 'Wavy_Hair', 'Young') and list(names[5:]) == sorted(names[5:], key=str.lower)
    assert sorted(ls.attribute_column(a) for a in range(40)) == list(range(40))
    assert all(CELEBA_ATTRIBUTES[ls.attribute_column(a)] == names[a] for a in range(40))
    assert ls.attribute_column(0) == 20 and ls.attribute_column(5) == 0


def test_ls_without_functions_and_without_a_pickle_raises_the_old_error(tmp_path, monkeypatch):
    from inclusivegan_amd.metrics import linear_separability as ls
    monkeypatch.chdir(tmp_path)                                         # no metrics/celeba_attribute_classifier.pkl here
    old = ('LS needs classify_fns: the reference\'s celebahq-classifier-00-male.pkl .. '
           'celebahq-classifier-39-wearing-necktie.pkl are not available in this tree')
    m = ls.LS(num_samples=8, num_keep=4, attrib_indices=[0, 1], minibatch_per_gpu=4, name='ls8')
    assert m.classifier_pkl == 'metrics/celeba_attribute_classifier.pkl' and m.classify_fns is None
    for metric in (m, ls.LS(num_samples=8, num_keep=4, attrib_indices=[0, 1], minibatch_per_gpu=4, name='ls8', classifier_pkl=str(tmp_path / 'absent.pkl')),
                   ls.LS(num_samples=8, num_keep=4, attrib_indices=[0, 1], minibatch_per_gpu=4, name='ls8', classifier_pkl=None)):
        with pytest.raises(RuntimeError) as e:
            metric._evaluate(None, {}, 1)
        assert str(e.value) == old
    # injected functions win: a pickle that could not even be opened is never looked at
    pkl = tmp_path / 'classifier.pkl'
    pkl.write_bytes(b'not a pickle: opening it would fail')
    fns = {0: None}
    m = ls.LS(num_samples=8, num_keep=4, attrib_indices=[0, 1], minibatch_per_gpu=4, name='ls8', classify_fns=fns, classifier_pkl=str(pkl))
    with pytest.raises(RuntimeError) as e:
        m._evaluate(None, {}, 1)                                        # attribute 1 has no function: the old error, not an unpickling error
    assert str(e.value) == old and m.classify_fns is fns


def test_parser_defaults():
    from inclusivegan_amd import train_classifier as TC
    a = TC.parse_args(['--data-dir', 'D', '--dataset', 'stacked_mnist_240k'])
    assert vars(a) == dict(data_dir='D', dataset='stacked_mnist_240k', out='metrics/stacked_mnist_classifier.pkl', kimg=600.0, minibatch=256,
                           lrate=0.002, holdout=10000, seed=0, fmap_base=1024, mode='digits', pos_weight='none')
    assert TC.parse_args(['--data-dir', 'D', '--dataset', 'X', '--mode', 'onehot']).out == 'metrics/stacked_mnist_classifier.pkl'
    a = TC.parse_args(['--data-dir', 'D', '--dataset', 'celeba_align_png_cropped_30k', '--mode', 'attributes'])
    assert a.out == 'metrics/celeba_attribute_classifier.pkl' and a.pos_weight == 'none' and (a.kimg, a.lrate) == (600.0, 0.002)
    assert TC.parse_args(['--data-dir', 'D', '--dataset', 'X', '--mode', 'attributes', '--pos-weight', 'balanced', '--out', 'o.pkl']).out == 'o.pkl'
    with pytest.raises(SystemExit):
        TC.parse_args(['--data-dir', 'D', '--dataset', 'X', '--pos-weight', 'balanced'])


def test_balanced_pos_weight():
    from inclusivegan_amd import train_classifier as TC
    labels = np.array([[1, 0, 1], [0, 0, 1], [0, 1, 0], [0, 0, 1]], np.float32)
    assert TC.balanced_pos_weight(labels).tolist() == [3.0, 3.0, np.float32(1 / 3)]
    for col in (np.ones(4, np.float32), np.zeros(4, np.float32)):
        bad = labels.copy()
        bad[:, 1] = col
        with pytest.raises(ValueError, match='attribute 1 has'):
            TC.balanced_pos_weight(bad)
