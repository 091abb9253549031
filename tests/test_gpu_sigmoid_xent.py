"""GPU: csrc/sigmoid_xent.hip (igan_sigmoid_xent_fwd / _bwd, igan_sigmoid_xent_stats_update, igan_binary_probs) against the
np.longdouble oracle of tests/bce_oracle.py, at (n, A) = (1, 1), (3, 40), (257, 40), (64, 64), (1031, 5): a single element, the
metric's width, a grid tail, an exact wave multiple, odd rows with only 4-byte alignment.  Logits are a seeded normal x 8 with
+-0, +-1e-30, the denormals, +-17, +-88, +-104, +-1e4 and +-fp32 max planted against both classes; targets mix 0, 1, -1 and NaN;
every case runs with and without pos_weight.

Bounds: loss, gradient and probabilities within 0.5 * spacing_fp32(ref) * (1 + 2^-20) of the unrounded oracle value -- the
kernels evaluate in fp64 and round once, and the margin covers the few-fp64-ulp error of the device's exp / log1p, far below it;
an infinite value is met exactly and a NaN by a NaN.  pred and the four counts exact; loss_sum bit-equal to a serial fp64 sum of
the returned fp32 losses in row order after two updates; ignored elements exactly +0 in loss and gradient and not counted; a
NaN or +-inf logit changes its own element only; two runs bit-identical."""
import numpy as np
import pytest
import torch

import bce_oracle as O

pytestmark = pytest.mark.gpu


def to(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_fwd(x, t, w, dev):
    from inclusivegan_amd import hip_ops
    loss, pred = hip_ops.sigmoid_xent_raw(to(x, dev), to(t, dev), to(w, dev))
    return loss.cpu().numpy(), pred.cpu().numpy()


def run_bwd(x, t, w, dloss, dev):
    from inclusivegan_amd import hip_ops
    return hip_ops.sigmoid_xent_bwd_raw(to(x, dev), to(t, dev), to(dloss, dev), to(w, dev)).cpu().numpy()


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'pos_weight'])
@pytest.mark.parametrize('n,A', O.SHAPES)
def test_forward_backward_probs_and_stats_against_the_oracle(cuda_device, n, A, weighted):
    from inclusivegan_amd import hip_ops
    seed = 100 * n + A
    x, t = O.logits_of(n, A, seed), O.targets_of(n, A, seed)
    w = O.pos_weight_of(A, seed) if weighted else None
    dloss = np.random.RandomState(seed + 1).randn(n, A).astype(np.float32)
    pos, neg = O.kinds(t)
    ignored = ~(pos | neg)

    want_loss, want_pred = O.forward(x, t, w)
    loss, pred = run_fwd(x, t, w, cuda_device)
    ok_l, r_l = O.within_half_spacing(loss, want_loss)
    want_d = O.backward(x, t, dloss, w)
    d = run_bwd(x, t, w, dloss, cuda_device)
    ok_d, r_d = O.within_half_spacing(d, want_d)
    want_p = O.binary_probs(x)
    probs = hip_ops.binary_probs(to(x, cuda_device))
    assert probs.is_contiguous() and tuple(probs.shape) == (A, n, 2)
    probs = probs.cpu().numpy()
    ok_p, r_p = O.within_half_spacing(probs, want_p)
    print('(%d, %d) %s: worst error / bound: loss %.4f, dlogits %.4f, probs %.4f' % (n, A, 'pos_weight' if weighted else 'plain', r_l, r_d, r_p))
    assert ok_l and ok_d and ok_p
    assert pred.dtype == np.int8 and np.array_equal(pred, want_pred)
    # ignored elements: exactly +0 in the loss and in the gradient
    assert loss[ignored].tobytes() == np.zeros(int(ignored.sum()), np.float32).tobytes()
    assert d[ignored].tobytes() == np.zeros(int(ignored.sum()), np.float32).tobytes()
    # two runs, identical bits
    loss2, pred2 = run_fwd(x, t, w, cuda_device)
    assert loss.tobytes() == loss2.tobytes() and pred.tobytes() == pred2.tobytes()
    assert d.tobytes() == run_bwd(x, t, w, dloss, cuda_device).tobytes()
    # the tick statistics: two calls accumulate; every column is the serial fp64 sum of the fp32 losses in row order
    st = hip_ops.BinaryXentStats(A, cuda_device)
    for _ in range(2):
        st.update(to(loss, cuda_device), to(x, cuda_device), to(t, cuda_device))
    got_sum, got_counts = st.sums()
    want_sum, want_counts = O.stats(np.concatenate([loss, loss]), np.concatenate([x, x]), np.concatenate([t, t]))
    assert np.array_equal(got_counts, want_counts) and int(got_counts.sum()) == 2 * int((pos | neg).sum())
    assert got_sum.tobytes() == want_sum.tobytes()
    mean, acc, bal = st.to_host()
    tp, fp, tn, fn = (want_counts[:, i].astype(np.float64) for i in range(4))
    with np.errstate(all='ignore'):
        assert np.array_equal(mean, want_sum / (tp + fp + tn + fn), equal_nan=True)
        assert np.array_equal(acc, (tp + tn) / (tp + fp + tn + fn), equal_nan=True)
        both = (tp + fn > 0) & (tn + fp > 0)
        assert np.array_equal(bal[both], 0.5 * (tp / (tp + fn) + tn / (tn + fp))[both])
    st.reset()
    assert not st.loss_sum.any() and not st.counts.any()


@pytest.mark.parametrize('n,A', [(3, 40), (257, 40), (1031, 5)])
def test_a_non_finite_logit_changes_its_own_element_only(cuda_device, n, A):
    from inclusivegan_amd import hip_ops
    rng = np.random.RandomState(n + A)
    x = (rng.randn(n, A) * 8).astype(np.float32)
    t = (rng.rand(n, A) < 0.5).astype(np.float32)
    w = O.pos_weight_of(A, 5)
    dloss = np.ones((n, A), np.float32)
    loss0, pred0 = run_fwd(x, t, w, cuda_device)
    d0 = run_bwd(x, t, w, dloss, cuda_device)
    p0 = hip_ops.binary_probs(to(x, cuda_device)).cpu().numpy()
    cells = [(0, 1), (n // 2, A // 2), (n - 1, A - 1), (n - 1, 0), (1, A - 2), (n // 3, 2)]
    values = [np.nan, np.inf, -np.inf, np.inf, -np.inf, np.nan]
    classes = [0.0, 1.0, 0.0, 0.0, 1.0, 1.0]                            # NaN, +inf and -inf each against a 0 and against a 1
    assert len(set(cells)) == len(cells)
    bad, tb = x.copy(), t.copy()
    for (r, c), v, cls in zip(cells, values, classes):
        bad[r, c], tb[r, c] = v, cls
    loss_c, pred_c = run_fwd(x, tb, w, cuda_device)                     # the clean run with the same targets
    d_c = run_bwd(x, tb, w, dloss, cuda_device)
    loss, pred = run_fwd(bad, tb, w, cuda_device)
    d = run_bwd(bad, tb, w, dloss, cuda_device)
    p = hip_ops.binary_probs(to(bad, cuda_device)).cpu().numpy()
    keep = np.ones((n, A), bool)
    for r, c in cells:
        keep[r, c] = False
    assert loss[keep].tobytes() == loss_c[keep].tobytes() and d[keep].tobytes() == d_c[keep].tobytes()
    assert pred[keep].tobytes() == pred_c[keep].tobytes() and p[keep.T].tobytes() == p0[keep.T].tobytes()
    assert loss0[keep].tobytes() == loss_c[keep].tobytes() and np.array_equal(pred0, pred_c) and d0[keep].tobytes() == d_c[keep].tobytes()
    want_loss, want_pred = O.forward(bad, tb, w)
    want_d, want_p = O.backward(bad, tb, dloss, w), O.binary_probs(bad)
    for r, c in cells:
        v, tv = bad[r, c], tb[r, c]
        if np.isnan(v):
            assert np.isnan(loss[r, c]) and np.isnan(d[r, c]) and pred[r, c] == 0 and np.all(np.isnan(p[c, r]))
        else:
            confident_right = (v > 0) == (tv == 1.0)
            assert loss[r, c] == (0.0 if confident_right else np.inf) and pred[r, c] == int(v > 0)
            assert d[r, c] == (0.0 if confident_right else (-w[c] if tv == 1.0 else 1.0))
            assert p[c, r].tolist() == ([1.0, 0.0] if v > 0 else [0.0, 1.0])
    assert np.array_equal(pred, want_pred)
    assert O.within_half_spacing(loss, want_loss)[0] and O.within_half_spacing(d, want_d)[0] and O.within_half_spacing(p, want_p)[0]
    # the statistics: the NaN stays in its column's sum
    st = hip_ops.BinaryXentStats(A, cuda_device)
    st.update(to(loss, cuda_device), to(bad, cuda_device), to(tb, cuda_device))
    got_sum, got_counts = st.sums()
    want_sum, want_counts = O.stats(loss, bad, tb)
    assert np.array_equal(got_counts, want_counts)
    assert np.array_equal(got_sum, want_sum, equal_nan=True) and np.isnan(got_sum[cells[0][1]])
    clean = np.setdiff1d(np.arange(A), [c for _, c in cells])
    assert np.all(np.isfinite(got_sum[clean])) and got_sum[clean].tobytes() == want_sum[clean].tobytes()


def test_autograd_function_and_double_backward(cuda_device):
    from inclusivegan_amd import hip_ops
    n, A = 17, 40
    x = to(O.logits_of(n, A, seed=9), cuda_device).requires_grad_(True)
    t = to(O.targets_of(n, A, seed=9), cuda_device)
    w = to(O.pos_weight_of(A, 9), cuda_device)
    g_out = torch.randn(n, A, device=cuda_device)
    for weight in (None, w):
        loss, pred = hip_ops.SigmoidXentFn.apply(x, t, weight)
        assert not pred.requires_grad and pred.dtype == torch.int8
        g, = torch.autograd.grad((loss * g_out).sum(), x)
        raw_loss, raw_pred = hip_ops.sigmoid_xent_raw(x.detach(), t, weight)
        assert torch.equal(loss.detach(), raw_loss) and torch.equal(pred, raw_pred)
        assert g.cpu().numpy().tobytes() == hip_ops.sigmoid_xent_bwd_raw(x.detach(), t, g_out, weight).cpu().numpy().tobytes()
        loss, _ = hip_ops.SigmoidXentFn.apply(x, t, weight)
        g, = torch.autograd.grad(loss.sum(), x, create_graph=True)
        with pytest.raises(NotImplementedError, match='second-order gradients are not built'):
            torch.autograd.grad(g.sum(), x)
    # the mean the trainer takes
    loss, _ = hip_ops.SigmoidXentFn.apply(x, t)
    g, = torch.autograd.grad(loss.mean(), x)
    want = O.backward(x.detach().cpu().numpy(), t.cpu().numpy(), np.full((n, A), np.float32(1.0 / (n * A)), np.float32))
    assert O.within_half_spacing(g.cpu().numpy(), want)[0]
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.sigmoid_xent_raw(torch.zeros(2, 3), torch.zeros(2, 3))


def test_buffers_that_are_only_4_byte_aligned(cuda_device):
    from inclusivegan_amd import hip_ops
    n, A = 33, 5
    x, t = O.logits_of(n, A, seed=7), O.targets_of(n, A, seed=7)
    want_loss, want_pred = run_fwd(x, t, None, cuda_device)
    want_p = hip_ops.binary_probs(to(x, cuda_device)).cpu().numpy()
    for lead in (1, 2, 3):
        views = []
        for a in (x, t):
            flat = torch.zeros(n * A + lead, device=cuda_device)
            flat[lead:] = to(a, cuda_device).reshape(-1)
            views.append(flat[lead:].view(n, A))
            assert views[-1].data_ptr() % 16 == 4 * lead
        loss, pred = hip_ops.sigmoid_xent_raw(*views)
        assert loss.cpu().numpy().tobytes() == want_loss.tobytes() and np.array_equal(pred.cpu().numpy(), want_pred)
        assert hip_ops.binary_probs(views[0]).cpu().numpy().tobytes() == want_p.tobytes()
