"""GPU: the batched HIP linear SVM (csrc/linear_svc.hip) and the linear separability metric on top of it.

The contract is the MINIMISER of the objective LinearSVC's defaults state, W* from the fp64 oracle of tests/ls_cases.py:
the GPU solve must be no farther from it than the reference's own call (d_ref of tests/golden/ls_golden.npz), meet
liblinear's stopping rule when its gradient is re-evaluated in fp64, and predict what W* predicts on every sample that is
not within reach of the weight difference (Cauchy-Schwarz: |dec_gpu - dec*| <= |W_gpu - W*| |(x, 1)|).

Measured on an MI355X, relative distance to W* (the bound d_ref in brackets): noisy 2.95e-08 (1.44e-05), separable_wide
3.88e-07 (6.84e-03), tails 6.75e-08 (9.54e-05); every band empty; also recorded in profiles/ls_svc.txt."""
import os

import numpy as np
import pytest
import torch

from tests import ls_cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ls_golden.npz')
BAND_CAP = 0.01
_fits = {}


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def gpu_fit(name, cuda_device):
    """(fit, predictions int32 [n, A]) of a case, solved once per process."""
    from inclusivegan_amd.metrics.linear_separability import linear_svc_fit, linear_svc_predict
    if name not in _fits:
        X, Y, _, _ = ls_cases.oracle(name)
        Xd = torch.from_numpy(X).to(cuda_device)
        fit = linear_svc_fit(Xd, Y)
        _fits[name] = (fit, linear_svc_predict(Xd, fit.W))
    return _fits[name]


def check_against_minimiser(tag, X, Y, W_gpu, pred, W_star, solved, d_ref):
    """Criteria (a) - (c); -> True when no sample of any attribute lies in the undecidable band."""
    dist = np.linalg.norm((W_gpu - W_star)[solved]) / np.linalg.norm(W_star[solved])
    print('%s: |W_gpu - W*| / |W*| = %.3e (d_ref %.3e)' % (tag, dist, d_ref))
    assert dist <= d_ref                                                                   # (a)
    rules = ls_cases.stopping_rule(X, Y, W_gpu)
    X1 = ls_cases.with_bias(X)
    xnorm = np.linalg.norm(X1, axis=1)
    empty = True
    for a in np.flatnonzero(solved):
        g, rule = rules[a]
        print('  attribute %d: fp64 |grad| %.3e, rule %.3e' % (a, g, rule))
        assert g <= rule                                                                   # (b)
        rows = Y[:, a] != 0
        dec = X1[rows] @ W_star[a]
        band = np.abs(dec) <= np.linalg.norm(W_gpu[a] - W_star[a]) * xnorm[rows]
        assert np.array_equal(pred[rows, a][~band], (dec > 0)[~band].astype(np.int32))     # (c)
        assert band.sum() <= BAND_CAP * rows.sum()
        empty &= not band.any()
    return empty


@pytest.mark.parametrize('name', sorted(ls_cases.SHAPES))
def test_solve_reaches_the_minimiser(name, golden, cuda_device):
    X, Y, W_star, solved = ls_cases.oracle(name)
    fit, pred = gpu_fit(name, cuda_device)
    assert fit.W.shape == W_star.shape and fit.W.dtype == np.float64 and pred.shape == Y.shape
    assert np.array_equal(fit.solved, solved) and fit.converged[solved].all() and not fit.converged[~solved].any()
    print('%s: Newton iterations %s' % (name, fit.n_iter.tolist()))
    if name in ('noisy', 'tails'):          # both cells of each column of the confusion table are populated
        dec = ls_cases.with_bias(X) @ W_star.T
        for a in np.flatnonzero(solved):
            rows = Y[:, a] != 0
            acc = np.mean((dec[rows, a] > 0) == (Y[rows, a] > 0))
            assert 0.6 < acc < 0.98, (a, acc)
    empty = check_against_minimiser(name, X, Y, fit.W, pred, W_star, solved, float(golden[name + '_d_ref']))

    # (d) with every band empty the (svm output, target) tables are the minimiser's, exactly
    if empty:
        from inclusivegan_amd.metrics.linear_separability import conditional_entropy, confusion_table
        for a in range(Y.shape[1]):
            rows = Y[:, a] != 0
            targets = (Y[rows, a] > 0).astype(np.int64)
            outputs = pred[rows, a] if fit.solved[a] else targets
            table = confusion_table(outputs, targets)
            assert np.array_equal(np.asarray(table, dtype=np.float64), golden[name + '_tables'][a]), a
            assert float(conditional_entropy(table)) == golden[name + '_cond_entropy'][a], a


def test_one_class_attribute_and_pruning(golden, cuda_device):
    """(e) the attribute whose kept targets hold one class is not solved; y = 0 rows change nothing: every attribute of
    `tails` solved alone on its compacted rows meets the same criteria."""
    from inclusivegan_amd.metrics.linear_separability import linear_svc_fit, linear_svc_predict
    X, Y, W_star, solved = ls_cases.oracle('tails')
    fit, _ = gpu_fit('tails', cuda_device)
    one = ls_cases.TAILS_ONE_CLASS
    assert not fit.solved[one] and not fit.converged[one] and fit.n_iter[one] == 0 and not fit.W[one].any()
    assert fit.solved.sum() == Y.shape[1] - 1
    d_ref = float(golden['tails_d_ref'])
    for a in range(Y.shape[1]):
        rows = Y[:, a] != 0
        Xa, Ya = np.ascontiguousarray(X[rows]), np.ascontiguousarray(Y[rows, a:a + 1])
        alone = linear_svc_fit(torch.from_numpy(Xa).to(cuda_device), Ya)
        assert bool(alone.solved[0]) == bool(solved[a])
        if not solved[a]:
            assert not alone.W.any() and alone.n_iter[0] == 0
            continue
        pred = linear_svc_predict(torch.from_numpy(Xa).to(cuda_device), alone.W)
        check_against_minimiser('tails[%d] alone' % a, Xa, Ya, alone.W, pred, W_star[a:a + 1], np.array([True]), d_ref)
        both = np.linalg.norm(alone.W[0] - fit.W[a]) / np.linalg.norm(W_star[a])
        print('  alone vs batched with y = 0 rows: %.3e' % both)
        assert both <= 2 * d_ref


@pytest.mark.parametrize('name', sorted(ls_cases.SHAPES))
def test_solve_is_repeatable_and_uncoupled(name, cuda_device):
    """(f) bit-identical W run to run, and with the attributes in reversed order (no cross-attribute coupling).

    Measured on an MI355X with the solver's fp64 vectors at their natural pitch F + 1: noisy and tails passed, separable_wide
    (pitch 513) was identical run to run but NOT under reversal.  The vectors are since padded to 16-element rows
    (linear_separability._Problem); that state has not been measured."""
    from inclusivegan_amd.metrics.linear_separability import linear_svc_fit
    X, Y, _, _ = ls_cases.oracle(name)
    fit, _ = gpu_fit(name, cuda_device)
    Xd = torch.from_numpy(X).to(cuda_device)
    again = linear_svc_fit(Xd, Y)
    assert np.array_equal(again.W, fit.W) and np.array_equal(again.n_iter, fit.n_iter)
    flipped = linear_svc_fit(Xd, np.ascontiguousarray(Y[:, ::-1]))
    assert np.array_equal(flipped.W[::-1], fit.W) and np.array_equal(flipped.n_iter[::-1], fit.n_iter)


def raw_case(kind):
    if kind == 'tails':
        X, Y, _, _ = ls_cases.oracle('tails')
        return X, Y
    n, F, A = kind
    rng = np.random.RandomState(n + F + A)
    X = rng.randn(n, F).astype(np.float32)
    Y = rng.randint(-1, 2, size=(n, A)).astype(np.int8)
    return X, Y


# tails: nothing a multiple of a tile.  The others walk the kernel's remaining paths: 4 / 3 column tiles per wave (fragments
# re-fetched per slab), float4 and scalar slab loads, all 64 attribute columns, two slabs per workgroup (n > 256 * 32).
@pytest.mark.parametrize('kind', ['tails', (300, 1000, 64), (130, 600, 33), (70, 771, 7), (8300, 8, 2)], ids=str)
def test_raw_passes_against_fp64(kind, cuda_device):
    """(g) gradient pass, Hessian-vector pass, line search and predictions at a random W and S."""
    from inclusivegan_amd import hip_ops
    X, Y = raw_case(kind)
    (n, F), A = X.shape, Y.shape[1]
    rng = np.random.RandomState(17)
    W = (rng.randn(A, F + 1) / np.sqrt(F)).astype(np.float32)
    S = (rng.randn(A, F + 1) / np.sqrt(F)).astype(np.float32)
    C = 1.0
    dev = cuda_device
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
    dec = torch.full((n, A), float('nan'), device=dev)
    z = torch.full((n, A), float('nan'), device=dev)
    act = torch.full((n, A), 7, device=dev, dtype=torch.uint8)
    loss, grad = hip_ops.linear_svc_grad_raw(Xd, Yd, torch.from_numpy(W).to(dev), dec, act, C)
    hv = hip_ops.linear_svc_hv_raw(Xd, act, torch.from_numpy(S).to(dev), z, C)
    t = torch.tensor([[1.0] * A, [0.3] * A, [0.0] * A], device=dev, dtype=torch.float64) * torch.linspace(0.5, 1.5, A, device=dev, dtype=torch.float64)
    vals = hip_ops.linear_svc_linesearch_raw(dec, z, Yd, t.contiguous())
    pred = hip_ops.linear_svc_predict_raw(dec)
    loss2, grad2 = hip_ops.linear_svc_grad_raw(Xd, Yd, torch.from_numpy(W).to(dev), torch.empty_like(dec), torch.empty_like(act), C)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)                         # same inputs, same bits
    dec, z, act, loss, grad, hv, vals, pred, t = (v.cpu().numpy() for v in (dec, z, act, loss, grad, hv, vals, pred, t))

    X1, y = ls_cases.with_bias(X), Y.astype(np.float64)
    dec64, z64 = X1 @ W.astype(np.float64).T, X1 @ S.astype(np.float64).T
    e_dec = np.abs(dec - dec64).max() / np.abs(dec64).max()
    e_z = np.abs(z - z64).max() / np.abs(z64).max()
    m64 = 1.0 - y * dec64
    on64 = (y != 0) & (m64 > 0)
    decided = np.abs(m64) > np.abs(dec - dec64).max()
    assert set(np.unique(act)) <= {0, 1} and np.array_equal(act.astype(bool)[decided], on64[decided])
    on = act.astype(bool)                       # the kernel's own mask: its sums are checked on the set it summed over
    assert (on != on64).sum() <= 0.001 * on.size
    loss64 = np.sum(np.where(on, m64, 0.0) ** 2, axis=0)
    grad64 = -2.0 * C * (np.where(on, y * m64, 0.0).T @ X1)
    hv64 = 2.0 * C * (np.where(on, z64, 0.0).T @ X1)
    e_loss = np.abs(loss - loss64).max() / np.abs(loss64).max()
    e_grad = np.linalg.norm(grad - grad64) / np.linalg.norm(grad64)
    e_hv = np.linalg.norm(hv - hv64) / np.linalg.norm(hv64)
    line64 = np.stack([np.sum(np.where(y != 0, np.maximum(0.0, 1.0 - y * (dec.astype(np.float64) + tk * z.astype(np.float64))), 0.0) ** 2, axis=0) for tk in t])
    e_line = (np.abs(vals - line64) / np.abs(line64)).max()
    print('%s: dec %.2e z %.2e loss %.2e grad %.2e hv %.2e line %.2e, mask differs on %d' % (kind, e_dec, e_z, e_loss, e_grad, e_hv, e_line, (on != on64).sum()))
    assert e_dec <= 1e-5 and e_z <= 1e-5
    assert e_loss <= 1e-5 and e_grad <= 1e-5 and e_hv <= 1e-5
    assert e_line <= 1e-6
    assert np.array_equal(pred, (dec > 0).astype(np.int32))


def test_metric_end_to_end(cuda_device, capsys):
    """(h) LS on the smallest G the suite builds; the reported _z and _w recomputed on the host from what the metric collected."""
    from inclusivegan_amd.dnnlib import tflib
    from inclusivegan_amd.metrics import linear_separability as ls
    from inclusivegan_amd.metrics import metric_base
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    from tests.ppl_oracle import FMAP_BASE, RES
    Gs = tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', seed=1,
                       num_channels=3, resolution=RES, label_size=0, fmap_base=FMAP_BASE, device=cuda_device)
    gen = torch.Generator().manual_seed(3)
    readouts = {a: torch.randn(3 * RES * RES, 1, generator=gen).to(cuda_device) for a in (3, 11, 20)}
    seen = []

    def classifier(a):
        def fn(images):
            seen.append(tuple(images.shape))
            flat = images.reshape(images.shape[0], -1)
            return (flat - flat.mean(dim=1, keepdim=True)) @ readouts[a]          # a fixed linear read-out of the image
        return fn

    args = dict(metric_defaults['ls'])
    args.update(num_samples=512, num_keep=256, attrib_indices=[3, 11, 20], minibatch_per_gpu=4, classify_fns={a: classifier(a) for a in readouts})
    metric = metric_base.MetricGroup([args]).metrics[0]
    assert type(metric) is ls.LS
    metric.run(Gs, num_gpus=1)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert [r.suffix for r in metric._results] == ['_z', '_w']
    z_val, w_val = (r.value for r in metric._results)
    assert line == metric.get_result_str().strip() and line.startswith('%-30s' % 'live-network')
    assert line.endswith(('ls_z %-10.4f ls_w %-10.4f' % (z_val, w_val)).strip())
    assert set(seen) == {(4, 3, RES, RES)}

    res = {k: v.cpu().numpy() for k, v in metric.results.items()}
    assert res['latents'].shape == (512, 512) and res['dlatents'].shape == (512, 512) and res[3].shape == (512, 2)
    assert np.allclose(res[11].sum(axis=1), 1.0, atol=1e-6)
    all_empty = True
    host = {}
    for space in ('latents', 'dlatents'):
        X = res[space]
        ces = []
        for j, a in enumerate([3, 11, 20]):
            kept = sorted(list(range(512)), key=lambda i: -np.max(res[a][i]))[:256]
            targets = np.argmax(res[a][kept], axis=1)
            y = (2 * targets - 1).astype(np.int8)
            assert (y > 0).any() and (y < 0).any()
            w_star = ls_cases.oracle_fit(X[kept], y)
            X1 = ls_cases.with_bias(X[kept])
            dec = X1 @ w_star
            w_gpu = metric.fits[space].W[j]
            band = np.abs(dec) <= np.linalg.norm(w_gpu - w_star) * np.linalg.norm(X1, axis=1)
            gpu_out = (X1 @ w_gpu > 0)
            assert np.array_equal(gpu_out[~band], (dec > 0)[~band]) and band.sum() <= BAND_CAP * 256
            all_empty &= not band.any()
            ces.append(ls.conditional_entropy(ls.confusion_table((dec > 0).astype(np.int64), targets)))
        host[space] = 2 ** np.sum(ces)
    print('ls end to end: _z %.6f _w %.6f, host %.6f %.6f, bands empty: %s' % (z_val, w_val, host['latents'], host['dlatents'], all_empty))
    if all_empty:
        assert abs(z_val - host['latents']) <= 1e-9 and abs(w_val - host['dlatents']) <= 1e-9
