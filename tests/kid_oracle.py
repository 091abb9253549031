"""Brute-force oracle of the KID kernel sums (csrc/poly_kernel_sum.hip, metrics/kernel_inception_distance.py), fp64 or better:
dot products from np.longdouble products, terms from the cube in np.longdouble, sums from math.fsum over each term's fp64
head and tail.  Test infrastructure only.

    k(a, b)  = (gamma * a.b + coef0)^3
    sums[s]  = (sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j)),   x_i = X[idx_x[s][i]], y_j = Y[idx_y[s][j]]
               i, j are POSITIONS: a row listed twice gives an off-diagonal pair

The error budget of an fp64 evaluation, a priori: with
    A(s, sum) = sum over the counted pairs of (|gamma| * sum_f |x_f * y_f| + |coef0|)^3
    bound     = (3 F + 9 + number of counted pairs) * 2^-53 * A
3 F covers the F products and additions of a dot product carried through the cube, 9 the multiply-add and the two products
of the cube with room to spare, and the pair count ANY order of adding the terms: the bound is derived, not measured, and does
not depend on the kernel's summation tree."""
import math

import numpy as np

U = 2.0 ** -53


def _fsum(terms):
    """The sum of np.longdouble terms to within an ulp of fp64: fsum over the fp64 head and tail of each."""
    terms = np.asarray(terms, np.longdouble).ravel()
    hi = terms.astype(np.float64)
    lo = (terms - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(list(hi) + list(lo))


def pair_terms(A, B, gamma, coef0):
    """k(a_i, b_j) for all rows of A and B -> np.longdouble [na, nb]."""
    A, B = np.asarray(A, np.float32).astype(np.longdouble), np.asarray(B, np.float32).astype(np.longdouble)
    v = np.longdouble(gamma) * (A @ B.T) + np.longdouble(coef0)
    return v * v * v


def pair_magnitudes(A, B, gamma, coef0):
    """(|gamma| * sum_f |a_f b_f| + |coef0|)^3 for all rows of A and B -> fp64 [na, nb]."""
    A, B = np.abs(np.asarray(A, np.float32).astype(np.float64)), np.abs(np.asarray(B, np.float32).astype(np.float64))
    v = abs(float(gamma)) * (A @ B.T) + abs(float(coef0))
    return v * v * v


def _one(A, B, gamma, coef0, skip_diagonal):
    terms, mags = pair_terms(A, B, gamma, coef0), pair_magnitudes(A, B, gamma, coef0)
    F, pairs = A.shape[1], terms.size
    if skip_diagonal:
        keep = ~np.eye(terms.shape[0], dtype=bool)
        terms, mags, pairs = terms[keep], mags[keep], int(keep.sum())
    return _fsum(terms), (3 * F + 9 + pairs) * U * math.fsum(mags.ravel())


def sums(X, Y, idx_x, idx_y, gamma, coef0):
    """-> (sums fp64 [S, 3], bounds fp64 [S, 3]) for index lists idx_x, idx_y [S, m] into X, Y."""
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    idx_x, idx_y = np.asarray(idx_x), np.asarray(idx_y)
    out, bound = np.empty((idx_x.shape[0], 3)), np.empty((idx_x.shape[0], 3))
    for s in range(idx_x.shape[0]):
        x, y = X[idx_x[s]], Y[idx_y[s]]
        for c, (a, b, skip) in enumerate(((x, x, True), (y, y, True), (x, y, False))):
            out[s, c], bound[s, c] = _one(a, b, gamma, coef0, skip)
    return out, bound


def diagonal_sums(X, idx_x, gamma, coef0):
    """sum_i k(x_i, x_i) per subset -> (fp64 [S], bounds fp64 [S]) with the budget of m counted pairs."""
    X, idx_x = np.asarray(X, np.float32), np.asarray(idx_x)
    out, bound = np.empty(idx_x.shape[0]), np.empty(idx_x.shape[0])
    for s in range(idx_x.shape[0]):
        x = X[idx_x[s]]
        terms, mags = np.diag(pair_terms(x, x, gamma, coef0)), np.diag(pair_magnitudes(x, x, gamma, coef0))
        out[s], bound[s] = _fsum(terms), (3 * x.shape[1] + 9 + terms.size) * U * math.fsum(mags)
    return out, bound


def kid(x, y):
    """KID of ONE subset pair by the published code: a = Kxx + Kyy, b = Kxy with k = (u.v / F + 1)^3 and
    (a.sum() - diag(a).sum()) / (m - 1) - 2 b.sum() / m, then / m; every sum exact (fsum)."""
    m, F = x.shape
    assert y.shape == (m, F)
    a = pair_terms(x, x, 1.0 / F, 1.0) + pair_terms(y, y, 1.0 / F, 1.0)
    b = pair_terms(x, y, 1.0 / F, 1.0)
    t = (np.longdouble(_fsum(a)) - np.longdouble(_fsum(np.diag(a)))) / (m - 1) - 2 * np.longdouble(_fsum(b)) / m
    return float(t / m)


def kid_of_subsets(X, Y, idx_x, idx_y):
    """Mean over the subsets of kid(X[idx_x[s]], Y[idx_y[s]]) -> (kid, per_subset t_s [S])."""
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    m = np.asarray(idx_x).shape[1]
    each = [kid(X[ix], Y[iy]) for ix, iy in zip(idx_x, idx_y)]
    return math.fsum(each) / len(each), np.asarray(each) * m


def kid_bound(bounds, m):
    """The sums' bounds carried into kid: (e_xx + e_yy) / (m (m - 1)) + 2 e_xy / m^2, averaged over the subsets."""
    bounds = np.asarray(bounds, np.float64)
    return float(np.mean((bounds[:, 0] + bounds[:, 1]) / (m * (m - 1.0)) + 2.0 * bounds[:, 2] / (m * float(m))))
