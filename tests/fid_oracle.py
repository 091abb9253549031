"""Host oracles and inputs for the streaming moments behind FID (csrc/moments.hip): the shifted sums and Gram matrix and the
mean / covariance in np.longdouble (x87 extended precision, 64-bit significand) from the same fp32 rows, the error bounds of
an n-term fp64 sum, and the two input families of the tests."""
import numpy as np

EPS50 = 2.0 ** -50      # n * EPS50 * sqrt(M_jj M_kk): worst case of an n-term fp64 sum (n * 2^-52 relative to the sum of
                        # absolute products, which Cauchy-Schwarz bounds by sqrt(M_jj M_kk)), times 4 for an fp64 BLAS oracle


def integer_rows(n, F):
    """Values 0 .. 15, asymmetric in row and column: every partial sum of the moments is an exact integer."""
    i = np.arange(n, dtype=np.int64)[:, None]
    j = np.arange(F, dtype=np.int64)[None, :]
    return ((7 * i + 3 * j + (i * j) % 5) % 16).astype(np.float32)


def float_rows(n, F, seed=0):
    """relu(N(0, 1) * exp(N(0, 1)) + 0.3): non-negative, heavy-tailed, a good share of exact zeros -- like a pooled activation."""
    rng = np.random.RandomState(seed)
    return np.maximum(rng.randn(n, F) * np.exp(rng.randn(n, F)) + 0.3, 0.0).astype(np.float32)


def first_rows_shift(X, rows=8):
    return X[:rows].astype(np.float64).mean(axis=0)


def shifted(X, shift):
    """d = (double)x - shift, rounded once to fp64: the kernel's operand."""
    D = X.astype(np.float64)
    return D if shift is None else D - np.asarray(shift, dtype=np.float64)[None, :]


def moments_fp64(X, shift):
    """(sum, gram) of the shifted rows with NumPy's fp64 statements (BLAS for the Gram matrix)."""
    D = shifted(X, shift)
    return D.sum(axis=0), D.T @ D


def moments_longdouble(X, shift, rows=None):
    """(sum [F], gram[rows, :]) in np.longdouble; `rows` None = every row of the Gram matrix."""
    D = shifted(X, shift).astype(np.longdouble)
    left = D if rows is None else D[:, rows]
    return D.sum(axis=0), left.T @ D


def mean_cov_longdouble(X):
    """Two-pass mean and covariance (np.cov's definition, rowvar=False) in np.longdouble."""
    L = X.astype(np.longdouble)
    mean = L.sum(axis=0) / L.shape[0]
    C = L - mean[None, :]
    return mean, (C.T @ C) / (L.shape[0] - 1)


def gram_bound(n, diag):
    """n * 2^-50 * sqrt(M_jj M_kk) for every (j, k); diag = the oracle's shifted Gram diagonal."""
    d = np.sqrt(np.asarray(diag, dtype=np.float64))
    return n * EPS50 * d[:, None] * d[None, :]


def sum_bound(n, diag):
    return n * EPS50 * np.sqrt(n * np.asarray(diag, dtype=np.float64))


def edge_rows(F, count=24, seed=0):
    """Row indices of the Gram matrix worth an extended-precision look: the tile edges (64) and a seeded sample."""
    fixed = [r for r in (0, 1, 15, 16, 31, 32, 63, 64, 65, 127, 128, F // 2, F - 65, F - 64, F - 2, F - 1) if 0 <= r < F]
    extra = np.random.RandomState(seed).randint(0, F, size=count).tolist()
    return np.array(sorted(set(fixed + extra)), dtype=np.int64)
