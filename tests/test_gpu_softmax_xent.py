"""GPU: csrc/softmax_xent.hip (igan_softmax_xent_fwd / _bwd, igan_xent_stats_update) against the fp64 oracle of
tests/xent_oracle.py.  Widths below, at and above a wavefront of columns, none a multiple of 4 except 64 and 1000 (rows are
unaligned); a single row, a ragged last workgroup (4 rows per workgroup), more rows than one workgroup holds.

Bounds (include/igan_hip.h states the arithmetic): lse against m + log S evaluated in np.longdouble (the NumPy fp64 statement
is itself up to 13 spacings of |lse| away from it where the sum cancels, so it cannot referee): within 4 fp64 spacings at |lse|
on every row whose addition does not cancel, and on the cancelling rows (|lse| < max(|m|, |log S|) / 2, decided from the
reference alone) within the bound xent_oracle.lse_reference derives from the arithmetic -- half a spacing at |lse|, one at
|log S| for the logarithm, (D + 3) 2^-53 for the sum -- both asserted, the worst ratio of each class printed (measured: 2.1 spacings, 0.15 of the derived bound); loss and every dlogits element
within 2 ulp of fp32 of the oracle value (the kernel computes in fp64 and rounds once, the second ulp covers the device's exp /
log); pred, the ignored rows and the counts exact; loss_sum within 2^-50 relative (an fp64 sum of the same fp32 terms in row
order); non-finite rows NaN and every other row bit-identical to a run without them; two runs bit-identical."""
import numpy as np
import pytest
import torch

import xent_oracle as O

pytestmark = pytest.mark.gpu


def run_fwd(x, labels, dev):
    from inclusivegan_amd import hip_ops
    loss, lse, pred = hip_ops.softmax_xent_raw(torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev))
    return loss.cpu().numpy(), lse.cpu().numpy(), pred.cpu().numpy()


def run_bwd(x, labels, lse, dloss, dev):
    from inclusivegan_amd import hip_ops
    to = lambda a: torch.from_numpy(a).to(dev)
    return hip_ops.softmax_xent_bwd_raw(to(x), to(labels), to(lse), to(dloss)).cpu().numpy()


@pytest.mark.parametrize('K', O.KS)
@pytest.mark.parametrize('n', O.NS)
def test_forward_backward_and_stats_against_fp64(cuda_device, n, K):
    from inclusivegan_amd import hip_ops
    for kind in O.KINDS:
        x = O.logits_of(kind, n, K, seed=100 * n + K)
        labels = O.labels_of(n, K, seed=n + K)
        dloss = np.random.RandomState(n * K).randn(n).astype(np.float32)
        want_loss, want_lse, want_pred = O.forward(x, labels)
        loss, lse, pred = run_fwd(x, labels, cuda_device)
        valid = (labels >= 0) & (labels < K)
        finite = np.isfinite(want_lse)
        assert np.array_equal(np.isnan(lse), np.isnan(want_lse)) and np.array_equal(pred, want_pred), kind
        assert np.array_equal(np.isnan(loss), np.isnan(want_loss)), kind
        ref_lse, lse_bound, cancelling = O.lse_reference(x)
        lse_err = np.abs((lse.astype(np.longdouble) - ref_lse).astype(np.float64))
        plain, cancel = finite & ~cancelling, finite & cancelling
        u_lse = float(np.max(lse_err[plain] / np.spacing(np.abs(want_lse[plain])), initial=0.0))      # fp64 spacings at |lse|: at most 4
        r_cancel = float(np.max(lse_err[cancel] / lse_bound[cancel], initial=0.0))                       # of the derived bound: at most 1
        u_loss = float(np.max(O.ulps32(loss[finite], want_loss[finite]), initial=0.0))
        want_d = O.backward(x, labels, want_lse, dloss)
        d = run_bwd(x, labels, lse, dloss, cuda_device)
        assert np.array_equal(np.isnan(d), np.isnan(want_d)), kind
        ok = ~np.isnan(want_d)
        u_d = float(np.max(O.ulps32(d[ok], want_d[ok]), initial=0.0))
        print('(%d, %d) %-8s: lse %.2f ulp64 on %d rows, %.3f of the derived bound on %d cancelling rows, loss %.2f ulp32, dlogits %.2f ulp32'
              % (n, K, kind, u_lse, int(plain.sum()), r_cancel, int(cancel.sum()), u_loss, u_d))
        assert u_lse <= 4 and r_cancel <= 1 and np.all(lse_err[finite] <= lse_bound[finite]), kind
        assert u_loss <= 2 and u_d <= 2, kind
        # ignored rows: exactly +0 in the loss and in every gradient element
        assert not np.any(loss[~valid]) and not np.any(d[~valid])
        # two runs, identical bits
        loss2, lse2, pred2 = run_fwd(x, labels, cuda_device)
        assert loss.tobytes() == loss2.tobytes() and lse.tobytes() == lse2.tobytes() and pred.tobytes() == pred2.tobytes()
        assert d.tobytes() == run_bwd(x, labels, lse, dloss, cuda_device).tobytes()
        # the tick statistics: two calls accumulate
        st = hip_ops.XentStats(K, cuda_device)
        to = lambda a: torch.from_numpy(a).to(cuda_device)
        for _ in range(2):
            st.update(to(loss), to(labels), to(pred))
        total, counted, correct = O.stats(np.concatenate([loss, loss]), np.concatenate([labels, labels]), np.concatenate([pred, pred]), K)
        got_total, got_counted, got_correct = st.sums()
        assert (got_counted, got_correct) == (counted, correct), kind
        if not np.isfinite(total):                   # a NaN row, or the +inf loss of a label at a -inf column
            assert np.isnan(got_total) if np.isnan(total) else got_total == total
        else:
            assert abs(got_total - total) <= 2.0 ** -50 * abs(total), (kind, got_total, total)
            if counted:
                assert st.to_host() == (got_total / counted, correct / counted)


@pytest.mark.parametrize('n,K', [(17, 10), (17, 65), (192, 1000), (5, 3)])
def test_non_finite_values_stay_in_their_row(cuda_device, n, K):
    x = O.logits_of('normal', n, K, seed=3)
    labels = np.random.RandomState(5).randint(K, size=n).astype(np.int32)
    dloss = np.ones(n, np.float32)
    loss0, lse0, pred0 = run_fwd(x, labels, cuda_device)
    d0 = run_bwd(x, labels, lse0, dloss, cuda_device)
    bad = x.copy()
    r_nan, r_inf, r_ninf = 1, n - 2, n // 2
    bad[r_nan, K // 2] = np.nan
    bad[r_inf, K - 1] = np.inf
    bad[r_ninf, :] = -np.inf
    loss, lse, pred = run_fwd(bad, labels, cuda_device)
    d = run_bwd(bad, labels, lse, dloss, cuda_device)
    rows = [r_nan, r_inf, r_ninf]
    others = np.setdiff1d(np.arange(n), rows)
    assert np.all(np.isnan(loss[rows])) and np.all(np.isnan(lse[rows])) and np.all(np.isnan(d[rows]))
    assert (pred[r_nan], pred[r_inf], pred[r_ninf]) == (K // 2, K - 1, 0)
    assert np.array_equal(pred, np.argmax(bad, axis=1))
    assert loss[others].tobytes() == loss0[others].tobytes() and lse[others].tobytes() == lse0[others].tobytes()
    assert d[others].tobytes() == d0[others].tobytes() and np.array_equal(pred[others], pred0[others])
    # a -inf among finite logits contributes exactly 0: the row is the row without that column
    if K > 1:
        y = x.copy()
        y[:, K - 1] = -np.inf
        lab = np.minimum(labels, K - 2)
        _, lse_y, _ = run_fwd(y, lab, cuda_device)
        ref_short, _, _ = O.lse_reference(np.ascontiguousarray(x[:, :K - 1]))
        _, bound, _ = O.lse_reference(y)
        assert np.all(np.abs((lse_y.astype(np.longdouble) - ref_short).astype(np.float64)) <= bound)
        dy = run_bwd(y, lab, lse_y, dloss, cuda_device)
        assert not np.any(dy[:, K - 1])


def test_autograd_function_and_double_backward(cuda_device):
    from inclusivegan_amd import hip_ops
    n, K = 17, 10
    x = torch.from_numpy(O.logits_of('normal', n, K, seed=9)).to(cuda_device).requires_grad_(True)
    labels = torch.from_numpy(O.labels_of(n, K, seed=9)).to(cuda_device)
    w = torch.randn(n, device=cuda_device)
    loss, pred = hip_ops.SoftmaxXentFn.apply(x, labels)
    assert not pred.requires_grad and pred.dtype == torch.int32
    g, = torch.autograd.grad((loss * w).sum(), x)
    raw_loss, lse, raw_pred = hip_ops.softmax_xent_raw(x.detach(), labels)
    assert torch.equal(loss.detach(), raw_loss) and torch.equal(pred, raw_pred)
    assert torch.equal(g, hip_ops.softmax_xent_bwd_raw(x.detach(), labels, lse, w))
    loss, _ = hip_ops.SoftmaxXentFn.apply(x, labels)
    g, = torch.autograd.grad(loss.sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match='second-order gradients are not built'):
        torch.autograd.grad(g.sum(), x)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.softmax_xent_raw(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.xent_stats_update_raw(torch.zeros(2), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                      torch.zeros(1, dtype=torch.float64), torch.zeros(2, dtype=torch.int64), 3)


def test_rows_that_are_only_4_byte_aligned(cuda_device):
    from inclusivegan_amd import hip_ops
    n, K = 33, 63
    x = O.logits_of('normal', n, K, seed=7)
    labels = O.labels_of(n, K, seed=7)
    want = run_fwd(x, labels, cuda_device)
    for lead in (1, 2, 3):
        flat = torch.zeros(n * K + lead, device=cuda_device)
        flat[lead:] = torch.from_numpy(x).to(cuda_device).reshape(-1)
        view = flat[lead:].view(n, K)
        assert view.data_ptr() % 16 == 4 * lead
        loss, lse, pred = hip_ops.softmax_xent_raw(view, torch.from_numpy(labels).to(cuda_device))
        assert loss.cpu().numpy().tobytes() == want[0].tobytes() and lse.cpu().numpy().tobytes() == want[1].tobytes()
        assert np.array_equal(pred.cpu().numpy(), want[2])
