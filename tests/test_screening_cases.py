"""Host: the inputs of tests/test_gpu_screening.py discriminate.  On flat rows a one-accumulator fp32 chain (screening_cases.chain_dots,
one or two products per accumulate step) leaves the statistical interval 2^-22 sqrt(dim) several times over, and a 1-NN screen
run on that interval drops the fp64 brute force's neighbour without measuring it; the interval the kernels use (nn1_tol, a
bound on any summation order) holds the same products with room.  On zero-mean rows the chain uses a twentieth of the
statistical interval: random rows cannot tell the two apart.  16 x 256 rows at dim 12 288: seconds."""
import functools

import numpy as np
import pytest

import screening_cases as S

NQ, NC, DIM = 16, 256, 12288
GPU_DIMS = (512, 768, 3072, 3073, 3076, 12288, 49152)
GPU_CUTS = ((16, 136), (72, 136), (72, 40), (72, 20), (24, 136), (72, 3))


@functools.lru_cache(maxsize=None)
def _model(family, n):
    q, c, ans = S.case(family, NQ, NC, DIM)
    return q, c, ans, S.chain_dots(q, c, n), S.row_sqnorm32(q), S.row_sqnorm32(c)


def test_nn1_tol_is_the_bound_of_the_header():
    """(dim + 2) u / (1 - (dim + 2) u) covers gamma_dim = dim u / (1 - dim u) for the product (any order of `dim` roundings,
    twice half of |q|^2 + |c|^2), u for the two norms' rounding to fp32, and the (1 - u) by which the kernels' t, formed from the
    rounded norms, can fall short."""
    u = S.U32
    for dim in (1, 7, 512, 3073, 12288, 49152, 1 << 20):
        gamma = dim * u / (1 - dim * u)
        assert S.nn1_tol(dim) * (1 - u) >= gamma + u
        assert S.nn1_tol(dim) >= S.statistical_tol(dim) or dim < 16
    assert S.nn1_tol(49152) < 3e-3


@pytest.mark.parametrize('n', [1, 2])
def test_flat_rows_break_a_statistical_interval(n):
    q, c, ans, dots, qn, cn = _model('flat', n)
    rho = S.interval_use(q, c, dots, qn, cn, d2=ans['d2'], tol=S.statistical_tol)
    keep = S.modelled_screen_keeps(q, c, dots, qn, cn, tol=S.statistical_tol)
    lost = int((~keep[np.arange(NQ), ans['nn_idx']]).sum())
    print('flat, %d product(s) per step: rho %.2f of the statistical interval, true neighbour dropped for %d of %d queries' % (n, rho.max(), lost, NQ))
    assert rho.max() > 1.0
    assert lost >= 1
    # the same products inside the interval the kernels use: nothing is dropped
    bound = S.interval_use(q, c, dots, qn, cn, d2=ans['d2'])
    print('                                of nn1_tol %.3f' % bound.max())
    assert bound.max() <= 0.5
    assert S.modelled_screen_keeps(q, c, dots, qn, cn)[np.arange(NQ), ans['nn_idx']].all()


def test_zero_mean_rows_do_not_discriminate():
    q, c, ans, dots, qn, cn = _model('zero_mean', 1)
    rho = S.interval_use(q, c, dots, qn, cn, d2=ans['d2'], tol=S.statistical_tol)
    print('zero_mean: rho %.4f of the statistical interval' % rho.max())
    assert rho.max() <= 0.1


def test_chain_model_is_a_sequential_fp32_sum():
    q, c, _ = S.case('positive', NQ, NC, 768)
    want = np.cumsum(q[3][None, :] * c, axis=1, dtype=np.float32)[:, -1]
    assert np.array_equal(S.chain_dots(q[3:4], c, 1)[0], want)


@pytest.mark.parametrize('dim', GPU_DIMS)
@pytest.mark.parametrize('family', S.FAMILIES)
def test_cases_are_decided_and_keep_their_duplicates(family, dim):
    """case() and cut() assert the decidedness condition and the planted duplicate pair themselves; here for every dim and cut the
    GPU module uses, so that a seed that does not meet it shows without a device."""
    q, c, ans = S.case(family, 72, 136, dim)
    assert q.dtype == c.dtype == np.float32 and q.shape == (72, dim) and c.shape == (136, dim)
    for nq, nc in GPU_CUTS:
        cq, cc, sub = S.cut(family, nq, nc, dim)
        assert np.array_equal(cc[1], cc[2]) and not np.array_equal(cc[0], cc[1])
        o = sub['knn_idx'][0].tolist()
        assert o.index(2) == o.index(1) + 1                      # query 0 meets the pair: the lower index first
        assert np.array_equal(sub['knn_idx'], np.argsort(sub['d2'], axis=1, kind='stable')[:, :sub['knn_idx'].shape[1]])
    if family in ('flat', 'flat_u8'):
        assert (q == q[:, :1]).all() and (c == c[:, :1]).all()
        level = np.abs(c[3:3 + 64, 0].reshape(8, 8) - q[:8, 0][None, :])      # slot s belongs to query (s - 3) % 8
        assert level.max() <= (2e-3 + 1e-6 if family == 'flat' else 2.0 / 255 + 1e-6)


def test_the_host_case_is_decided_too():
    for family in S.FAMILIES:
        S.case(family, NQ, NC, DIM)
    assert set(S.cases(NQ, NC, DIM)) == set(S.FAMILIES)
