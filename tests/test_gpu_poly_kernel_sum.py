"""GPU: igan_poly3_kernel_sums (csrc/poly_kernel_sum.hip) through hip_ops.poly3_kernel_sums against the brute force of
tests/kid_oracle.py.  Every sum of every subset is held to the oracle's a-priori budget
    (3 F + 9 + counted pairs) * 2^-53 * sum over the counted pairs of (|gamma| sum_f |x_f y_f| + |coef0|)^3
which covers any summation order; bitwise statements (independence of the other subsets, of the run and of the workspace's
contents, non-finite rows) compare tobytes().  Sizes: tile tails in both directions (m = 63, 65, 130 against the 64 x 64 tile),
a single symmetric tile, a 3 x 3 tile triangle (m = 130), a K-chunk tail (F = 33, 100, 257 against 32) and F below one k-step."""
import functools

import numpy as np
import pytest
import torch

import kid_oracle

pytestmark = pytest.mark.gpu

NX, NY = 150, 141


def run(dev, X, Y, ix, iy, gamma, coef0, same=False, workspace=None):
    from inclusivegan_amd import hip_ops
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    Yd = Xd if same else torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
    out = hip_ops.poly3_kernel_sums(Xd, Yd, ix, iy, gamma, coef0, workspace=workspace)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(ix), 3) and out.is_cuda
    return out.cpu().numpy()


def within(got, want, bound):
    """|got - want| <= bound, entry by entry, the difference taken in extended precision; -> the largest share of the budget used."""
    err = np.abs(got.astype(np.longdouble) - want.astype(np.longdouble)).astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (err / bound).max()
    return float((err / bound).max())


@functools.lru_cache(maxsize=None)
def case(m, F, S=3):
    """Signed features, distinct nx != ny, S subsets drawn without replacement; the oracle's sums and bounds; shared, never written to."""
    rng = np.random.RandomState(1000 * m + F)
    X = rng.randn(NX, F).astype(np.float32)
    Y = (rng.randn(NY, F) + 0.5).astype(np.float32)
    ix = np.stack([rng.choice(NX, m, replace=False) for _ in range(S)])
    iy = np.stack([rng.choice(NY, m, replace=False) for _ in range(S)])
    want, bound = kid_oracle.sums(X, Y, ix, iy, 1.0 / F, 1.0)
    for a in (X, Y, ix, iy, want, bound):
        a.setflags(write=False)
    return X, Y, ix, iy, want, bound


@pytest.mark.parametrize('F', [1, 3, 31, 33, 100, 257])
@pytest.mark.parametrize('m', [2, 3, 63, 64, 65, 130])
def test_sums_within_the_budget(cuda_device, m, F):
    X, Y, ix, iy, want, bound = case(m, F)
    got = run(cuda_device, X, Y, ix, iy, 1.0 / F, 1.0)
    print('m %d F %d: share of the budget used %.3g' % (m, F, within(got, want, bound)))


def test_sums_at_the_metric_width(cuda_device):
    X, Y, ix, iy, want, bound = case(130, 2048, S=2)
    got = run(cuda_device, X, Y, ix, iy, 1.0 / 2048, 1.0)
    print('m 130 F 2048: share of the budget used %.3g' % within(got, want, bound))


def test_other_gamma_and_coef0(cuda_device):
    X, Y, ix, iy, _, _ = case(65, 33)
    for gamma, coef0 in ((0.25, 0.0), (-0.5, 2.0), (1.0 / 33, -1.0)):
        want, bound = kid_oracle.sums(X, Y, ix, iy, gamma, coef0)
        within(run(cuda_device, X, Y, ix, iy, gamma, coef0), want, bound)


def test_the_diagonal_is_one_of_positions_not_of_rows(cuda_device):
    """Subset 1 lists row 7 twice (positions 4 and 40): k(x_7, x_7) enters its symmetric sum twice, as the oracle counts it."""
    X, Y, ix, iy, _, _ = case(65, 33)
    ix = np.array(ix)
    ix[1] = np.where(ix[1] == 7, 8, ix[1])
    ix[1, 4] = ix[1, 40] = 7
    want, bound = kid_oracle.sums(X, Y, ix, iy, 1.0 / 33, 1.0)
    got = run(cuda_device, X, Y, ix, iy, 1.0 / 33, 1.0)
    within(got, want, bound)
    # the statement has teeth: dropping the two cells moves the sum by far more than the budget
    k77 = float(kid_oracle.pair_terms(X[7:8], X[7:8], 1.0 / 33, 1.0)[0, 0])
    assert 2 * k77 > 1000 * bound[1, 0]


def test_same_set_on_both_sides(cuda_device):
    """X and Y the same tensor, idx_x == idx_y: the cross sum is the symmetric sum plus the diagonal."""
    X, _, ix, _, _, _ = case(130, 100)
    want, bound = kid_oracle.sums(X, X, ix, ix, 0.01, 1.0)
    got = run(cuda_device, X, None, ix, ix, 0.01, 1.0, same=True)
    within(got, want, bound)
    assert got[:, 0].tobytes() == got[:, 1].tobytes()
    diag, _ = kid_oracle.diagonal_sums(X, ix, 0.01, 1.0)
    err = np.abs(got[:, 2].astype(np.longdouble) - got[:, 0].astype(np.longdouble) - diag.astype(np.longdouble)).astype(np.float64)
    assert np.all(err <= bound[:, 2] + bound[:, 0]), err / (bound[:, 2] + bound[:, 0])


def cancelling_rows(rng, n, F):
    """Rows 1 + j 2^-23 with small integers j: with gamma = 1 / F and coef0 = -1 the kernel's base gamma x.y + coef0 is
    (sum of the j's of both rows) 2^-23 / F + O(2^-46), tiny and of either sign.  The j of a row have mean +1, or -1 for a third
    of the rows: a pair of two such rows is negative, a mixed pair half of the time -- a third of all pairs."""
    j = rng.randint(-3, 6, size=(n, F)) - (rng.rand(n, 1) < 1.0 / 3.0) * 2
    return (1.0 + j * 2.0 ** -23).astype(np.float32)


def test_cancellation_and_a_wide_range(cuda_device):
    F, m = 33, 65
    rng = np.random.RandomState(77)
    X, Y = cancelling_rows(rng, NX, F), cancelling_rows(rng, NY, F)
    base = (X.astype(np.float64) @ Y.astype(np.float64).T) / F - 1.0
    share = float((base < 0).mean())
    print('base within %.3g of 0, negative for %.3f of the pairs' % (np.abs(base).max(), share))
    assert np.abs(base).max() < 1e-6 and 0.25 <= share <= 0.42
    ix = np.stack([rng.choice(NX, m, replace=False) for _ in range(3)])
    iy = np.stack([rng.choice(NY, m, replace=False) for _ in range(3)])
    want, bound = kid_oracle.sums(X, Y, ix, iy, 1.0 / F, -1.0)
    assert np.all(np.abs(want) < 1e-14)                    # sums of cubes of 1e-7: everything but the last bits of a dot cancels
    within(run(cuda_device, X, Y, ix, iy, 1.0 / F, -1.0), want, bound)
    # rows of magnitude 1e4 (cubes near 1e24) next to rows of 1e-4, in the same subsets
    X, Y = np.array(X), np.array(Y)
    X[ix[0, :5]] = (1e4 * (1 + rng.rand(5, F))).astype(np.float32)
    Y[iy[0, :5]] = (1e4 * (1 + rng.rand(5, F))).astype(np.float32)
    X[ix[0, 5:10]] = (1e-4 * rng.randn(5, F)).astype(np.float32)
    Y[iy[1, :5]] = (-1e4 * (1 + rng.rand(5, F))).astype(np.float32)
    want, bound = kid_oracle.sums(X, Y, ix, iy, 1.0 / F, -1.0)
    assert np.abs(want).max() > 1e24
    within(run(cuda_device, X, Y, ix, iy, 1.0 / F, -1.0), want, bound)


def test_a_subset_does_not_depend_on_the_others_the_run_or_the_workspace(cuda_device):
    from inclusivegan_amd import _abi
    X, Y, ix, iy, want, bound = case(130, 100)
    whole = run(cuda_device, X, Y, ix, iy, 0.01, 1.0)
    within(whole, want, bound)
    assert run(cuda_device, X, Y, ix, iy, 0.01, 1.0).tobytes() == whole.tobytes()
    for s in range(3):
        alone = run(cuda_device, X, Y, ix[s:s + 1], iy[s:s + 1], 0.01, 1.0)
        assert alone.tobytes() == whole[s:s + 1].tobytes(), s
    assert run(cuda_device, X, Y, ix[::-1], iy[::-1], 0.01, 1.0).tobytes() == whole[::-1].tobytes()
    nbytes = int(_abi.get_plugin().igan_poly3_kernel_sums_workspace_bytes(3, 130))
    assert nbytes == 3 * (6 + 6 + 9) * 8
    garbage = torch.full((nbytes // 8 + 5,), float('nan'), device=cuda_device, dtype=torch.float64)
    assert run(cuda_device, X, Y, ix, iy, 0.01, 1.0, workspace=garbage).tobytes() == whole.tobytes()
    with pytest.raises(ValueError, match='workspace'):
        run(cuda_device, X, Y, ix, iy, 0.01, 1.0, workspace=garbage[:nbytes // 8 - 1].contiguous())


@pytest.mark.parametrize('side, value', [('x', float('nan')), ('y', float('inf'))])
def test_a_non_finite_row_reaches_the_subsets_that_list_it(cuda_device, side, value):
    """One element of one row: non-finite in exactly the two sums of the subsets that list the row, every other entry
    bit-identical to the clean run.  (The +inf row sits among non-negative rows: inf * 0 would be a NaN all the same.)"""
    m, F = 65, 33
    rng = np.random.RandomState(9)
    X, Y = np.abs(rng.randn(NX, F)).astype(np.float32), np.abs(rng.randn(NY, F)).astype(np.float32)
    ix = np.stack([rng.choice(NX, m, replace=False) for _ in range(4)])
    iy = np.stack([rng.choice(NY, m, replace=False) for _ in range(4)])
    idx = ix if side == 'x' else iy
    row = next(r for r in idx[1] if r not in idx[0] and r not in idx[3])          # listed by subset 1, not by 0 and 3
    listed = np.array([row in idx[s] for s in range(4)])
    assert listed[1] and not listed[0] and not listed[3]
    clean = run(cuda_device, X, Y, ix, iy, 1.0 / F, 1.0)
    dirty_in = np.array(X if side == 'x' else Y)
    dirty_in[row, 17] = value
    got = run(cuda_device, dirty_in if side == 'x' else X, Y if side == 'x' else dirty_in, ix, iy, 1.0 / F, 1.0)
    touched = np.zeros((4, 3), bool)
    touched[listed, 0 if side == 'x' else 1] = True
    touched[listed, 2] = True
    assert np.all(np.isnan(got[touched])) if np.isnan(value) else np.all(np.isposinf(got[touched]))
    assert np.all(np.isfinite(got[~touched]))
    assert got[~touched].tobytes() == clean[~touched].tobytes()


def fp32_statement(dev, X, Y, ix, iy, gamma, coef0):
    """The same three sums as torch fp32 statements on `dev`: mm, scale, add, cube, sum; the diagonal subtracted."""
    out = np.empty((len(ix), 3))
    Xd, Yd = torch.from_numpy(np.ascontiguousarray(X)).to(dev), torch.from_numpy(np.ascontiguousarray(Y)).to(dev)

    def total(a, b, skip):
        K = (torch.mm(a, b.t()) * np.float32(gamma) + np.float32(coef0)) ** 3
        assert K.dtype == torch.float32
        return float(K.sum() - torch.diagonal(K).sum()) if skip else float(K.sum())

    for s in range(len(ix)):
        x, y = Xd[torch.from_numpy(ix[s]).to(dev)], Yd[torch.from_numpy(iy[s]).to(dev)]
        out[s] = [total(x, x, True), total(y, y, True), total(x, y, False)]
    return out


def test_not_fp32(cuda_device):
    """Non-negative rows, F = 257, m = 130: the kernel sits inside the budget; the fp32 statement of the same sums misses every
    one of them by at least 1000 budgets (on the CPU, where the input was chosen: 18 000 to 63 000 budgets; and on the device).
    A kernel that formed fp32 products or fp32 sums would fail the first assertion."""
    F, m = 257, 130
    rng = np.random.RandomState(0)
    X = np.abs(rng.randn(NX, F)).astype(np.float32)
    Y = np.abs(rng.randn(NY, F) + 0.3).astype(np.float32)
    ix = np.stack([rng.choice(NX, m, replace=False) for _ in range(2)])
    iy = np.stack([rng.choice(NY, m, replace=False) for _ in range(2)])
    want, bound = kid_oracle.sums(X, Y, ix, iy, 1.0 / F, 1.0)
    used = within(run(cuda_device, X, Y, ix, iy, 1.0 / F, 1.0), want, bound)
    for dev in ('cpu', cuda_device):
        miss = np.abs(fp32_statement(dev, X, Y, ix, iy, 1.0 / F, 1.0) - want) / bound
        print('%s fp32 statement misses by %s budgets; the kernel uses %.3g of one' % (dev, np.round(miss).tolist(), used))
        assert np.all(miss >= 1000.0)
