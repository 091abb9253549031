"""Inputs and the fp64 oracle shared by tests/golden/make_ls_golden.py, tests/test_linear_separability.py and
tests/test_gpu_linear_separability.py: seeded sample matrices X [n, F] fp32 with targets Y [n, A] in {-1, 0, +1} (0 = the
attribute has pruned the sample), and a NumPy Newton solve of the objective LinearSVC's defaults state,

    f(w) = 1/2 |w|^2 + C * sum_i max(0, 1 - y_i * w.(x_i, 1))^2,        w in R^(F+1), the bias last,

to |grad f| <= 1e-12 |grad f(0)|: the minimiser every solver is measured against, available where sklearn is not."""
import numpy as np

SHAPES = {'noisy': (3000, 48, 3), 'separable_wide': (1500, 512, 40), 'tails': (777, 37, 5)}
TAILS_ONE_CLASS, TAILS_ALL_KEPT = 3, 0
_cache = {}


def make_case(name):
    """-> X float32 [n, F], Y int8 [n, A]."""
    n, F, A = SHAPES[name]
    if name == 'noisy':          # labels = sign(X.t + 0.5 noise + 0.3): not separable, every sample kept
        rng = np.random.RandomState(101)
        X = rng.randn(n, F).astype(np.float32)
        t = rng.randn(F, A) / np.sqrt(F)
        s = X.astype(np.float64) @ t + 0.5 * rng.randn(n, A) + 0.3
        return X, np.where(s > 0, 1, -1).astype(np.int8)
    if name == 'separable_wide':  # no label noise, F above one 32-column tile and above one tile per wave
        rng = np.random.RandomState(202)
        X = rng.randn(n, F).astype(np.float32)
        t = rng.randn(F, A) / np.sqrt(F)
        s = X.astype(np.float64) @ t + 0.2
        return X, np.where(s > 0, 1, -1).astype(np.int8)
    if name == 'tails':           # nothing a multiple of a tile; anisotropic, off-centre samples; per-attribute pruning masks
        rng = np.random.RandomState(303)
        X = (rng.randn(n, F) * np.exp(0.5 * rng.randn(F)) + 0.25 * rng.randn(F)).astype(np.float32)
        t = rng.randn(F, A) / np.sqrt(F)
        s = X.astype(np.float64) @ t + 0.5 * rng.randn(n, A) * np.std(X.astype(np.float64) @ t, axis=0) + 0.3
        Y = np.where(s > 0, 1, -1).astype(np.int8)
        for a in range(A):
            if a != TAILS_ALL_KEPT:
                Y[rng.permutation(n)[:n // 2], a] = 0        # half of the samples pruned, another half per attribute
        Y[:, TAILS_ONE_CLASS] = np.abs(Y[:, TAILS_ONE_CLASS])  # the kept targets of this attribute hold one class
        return X, Y
    raise KeyError(name)


def with_bias(X):
    return np.hstack([np.asarray(X, dtype=np.float64), np.ones((X.shape[0], 1))])


def objective(X1, y, w, C=1.0):
    """f, grad f and the active mask at w (fp64; X1 carries the bias column, y in {-1, +1})."""
    m = 1.0 - y * (X1 @ w)
    on = m > 0
    return 0.5 * w @ w + C * np.sum(m[on] ** 2), w - 2.0 * C * (X1[on].T @ (y[on] * m[on])), on


def oracle_fit(X, y, C=1.0, rel=1e-12, max_iter=200):
    """Newton with the exact generalised Hessian I + 2C X_on^T X_on and Armijo backtracking -> w [F + 1]."""
    X1, y = with_bias(X), np.asarray(y, dtype=np.float64)
    w = np.zeros(X1.shape[1])
    f, g, on = objective(X1, y, w, C)
    g0 = np.linalg.norm(g)
    for _ in range(max_iter):
        if np.linalg.norm(g) <= rel * g0:
            break
        s = np.linalg.solve(np.eye(len(w)) + 2.0 * C * (X1[on].T @ X1[on]), -g)
        t = 1.0
        while True:
            fn, gn, onn = objective(X1, y, w + t * s, C)
            if fn <= f + 1e-4 * t * (g @ s) or t < 1e-12:
                break
            t *= 0.5
        w, f, g, on = w + t * s, fn, gn, onn
    assert np.linalg.norm(g) <= rel * g0, 'the oracle did not converge'
    return w


def oracle_fit_all(X, Y, C=1.0):
    """Every attribute on its compacted rows -> W [A, F + 1] (zero rows where the kept targets hold one class), solved [A]."""
    W = np.zeros((Y.shape[1], X.shape[1] + 1))
    solved = np.zeros(Y.shape[1], dtype=bool)
    for a in range(Y.shape[1]):
        rows = Y[:, a] != 0
        y = Y[rows, a]
        solved[a] = (y > 0).any() and (y < 0).any()
        if solved[a]:
            W[a] = oracle_fit(X[rows], y, C)
    return W, solved


def oracle(name):
    """(X, Y, W*, solved) of a case, computed once per process and never modified."""
    if name not in _cache:
        X, Y = make_case(name)
        W, solved = oracle_fit_all(X, Y)
        for arr in (X, Y, W, solved):
            arr.setflags(write=False)
        _cache[name] = (X, Y, W, solved)
    return _cache[name]


def stopping_rule(X, Y, W, tol=1e-4, C=1.0):
    """liblinear's primal rule in fp64: (|grad f_a(W_a)|, tol * max(min(pos, neg), 1) / l * |grad f_a(0)|) per attribute."""
    out = []
    for a in range(Y.shape[1]):
        rows = Y[:, a] != 0
        X1, y = with_bias(X[rows]), Y[rows, a].astype(np.float64)
        g = objective(X1, y, np.asarray(W[a], dtype=np.float64), C)[1]
        g0 = objective(X1, y, np.zeros(X1.shape[1]), C)[1]
        pos, neg = int((y > 0).sum()), int((y < 0).sum())
        out.append((np.linalg.norm(g), tol * max(min(pos, neg), 1) / max(len(y), 1) * np.linalg.norm(g0)))
    return out
