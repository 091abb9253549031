"""fp64 NumPy restatements of the differentiable augmentation (inclusivegan_amd/training/augment.py states the contract), shared
by tests/test_diffaugment.py and tests/test_gpu_diffaugment.py.  Nothing here imports the package.

  forward_loops       the contract form, pixel by pixel
  forward_sequential  brightness, then saturation, then contrast applied one after another, each with the mean it sees, then a
                      zero-padded shift, then the cutout: another route to the same numbers (it shows the mean identity)
  forward64 / transpose64   the contract form and its transpose on whole arrays, for the larger shapes of the GPU tests
                      (test_diffaugment.py holds forward64 to forward_loops)

Integer parameters come from the fp32 product in every form: that is part of the contract, not of the arithmetic under test."""
import numpy as np

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
EDGE_U = (0.0, 0.5, float(np.nextafter(np.float32(1), np.float32(0))))


def draw(u, k):
    return min(int(np.floor(np.float32(u) * np.float32(k))), k - 1)


def geometry(urow, H, W, bits):
    """(t_y, t_x, cut rows [y0, y1), cut columns [x0, x1)) -- the cut ranges NOT intersected with the image; empty without cutout."""
    ty = tx = 0
    y0 = y1 = x0 = x1 = 0
    if bits & TRANSLATION:
        Sy, Sx = int(np.floor(H / 8 + 0.5)), int(np.floor(W / 8 + 0.5))
        ty = draw(urow[4], 2 * Sy + 1) - Sy
        tx = draw(urow[3], 2 * Sx + 1) - Sx
    if bits & CUTOUT:
        Ky, Kx = int(np.floor(H / 2 + 0.5)), int(np.floor(W / 2 + 0.5))
        y0 = draw(urow[6], H + 1 - Ky % 2) - Ky // 2
        x0 = draw(urow[5], W + 1 - Kx % 2) - Kx // 2
        y1, x1 = y0 + Ky, x0 + Kx
    return ty, tx, y0, y1, x0, x1


def color_params(urow):
    u = np.asarray(urow, np.float32).astype(np.float64)
    return u[0] - 0.5, 2.0 * u[1], u[2] + 0.5


def zero_mask(u, shape, bits):
    """True where the contract makes the forward output exactly 0: cut, or shifted in from outside the image."""
    n, C, H, W = shape
    z = np.zeros(shape, bool)
    i, j = np.arange(H).reshape(H, 1), np.arange(W).reshape(1, W)
    for k in range(n):
        ty, tx, y0, y1, x0, x1 = geometry(u[k], H, W, bits)
        cut = (y0 <= i) & (i < y1) & (x0 <= j) & (j < x1)
        inside = (0 <= i + ty) & (i + ty < H) & (0 <= j + tx) & (j + tx < W)
        z[k] = cut | ~inside
    return z


def forward_loops(x, u, bits):
    x = np.asarray(x, np.float64)
    n, C, H, W = x.shape
    y = np.zeros_like(x)
    for k in range(n):
        ty, tx, y0, y1, x0, x1 = geometry(u[k], H, W, bits)
        b, s, c = color_params(u[k])
        m = x[k].sum() / (C * H * W)
        M = m + b
        for i in range(H):
            for j in range(W):
                si, sj = i + ty, j + tx
                if (y0 <= i < y1 and x0 <= j < x1) or not (0 <= si < H and 0 <= sj < W):
                    continue
                px = x[k, :, si, sj]
                if bits & COLOR:
                    p = (px + b).sum() / C
                    px = ((px + b - p) * s + p - M) * c + M
                y[k, :, i, j] = px
    return y


def forward_sequential(x, u, bits):
    x = np.asarray(x, np.float64)
    n, C, H, W = x.shape
    y = np.zeros_like(x)
    for k in range(n):
        ty, tx, y0, y1, x0, x1 = geometry(u[k], H, W, bits)
        v = x[k].copy()
        if bits & COLOR:
            b, s, c = color_params(u[k])
            v = v + b                                              # brightness
            pm = v.mean(axis=0, keepdims=True)
            v = (v - pm) * s + pm                                  # saturation about every pixel's channel mean
            mm = v.mean()
            v = (v - mm) * c + mm                                  # contrast about the mean of what it is given
        pad_y, pad_x = abs(ty), abs(tx)
        padded = np.zeros((C, H + 2 * pad_y, W + 2 * pad_x))
        padded[:, pad_y:pad_y + H, pad_x:pad_x + W] = v
        w = padded[:, pad_y + ty:pad_y + ty + H, pad_x + tx:pad_x + tx + W].copy()
        for i in range(max(y0, 0), min(y1, H)):
            for j in range(max(x0, 0), min(x1, W)):
                w[:, i, j] = 0.0
        y[k] = w
    return y


def _shift(v, ty, tx):
    """w(i, j) = v(i + ty, j + tx) inside the image, else 0, for v [C, H, W]."""
    C, H, W = v.shape
    w = np.zeros_like(v)
    i0, i1 = max(0, -ty), min(H, H - ty)
    j0, j1 = max(0, -tx), min(W, W - tx)
    if i0 < i1 and j0 < j1:
        w[:, i0:i1, j0:j1] = v[:, i0 + ty:i1 + ty, j0 + tx:j1 + tx]
    return w


def forward64(x, u, bits):
    x = np.asarray(x, np.float64)
    n, C, H, W = x.shape
    y = np.empty_like(x)
    for k in range(n):
        ty, tx, y0, y1, x0, x1 = geometry(u[k], H, W, bits)
        v = x[k]
        if bits & COLOR:
            b, s, c = color_params(u[k])
            M = v.sum() / (C * H * W) + b
            p = (v + b).sum(axis=0, keepdims=True) / C
            v = ((v + b - p) * s + p - M) * c + M
        w = _shift(v, ty, tx)
        w[:, max(y0, 0):max(min(y1, H), 0), max(x0, 0):max(min(x1, W), 0)] = 0.0
        y[k] = w
    return y


def transpose64(dy, u, bits):
    dy = np.asarray(dy, np.float64)
    n, C, H, W = dy.shape
    dx = np.empty_like(dy)
    for k in range(n):
        ty, tx, y0, y1, x0, x1 = geometry(u[k], H, W, bits)
        d = dy[k].copy()
        d[:, max(y0, 0):max(min(y1, H), 0), max(x0, 0):max(min(x1, W), 0)] = 0.0
        g = _shift(d, -ty, -tx)                                    # g(i, j) = dy(i - t_y, j - t_x)
        if bits & COLOR:
            b, s, c = color_params(u[k])
            q = g.sum(axis=0, keepdims=True) / C
            g = c * s * g + c * (1 - s) * q + (1 - c) * g.sum() / (C * H * W)
        dx[k] = g
    return dx


def u_rows(n, seed):
    """Pool of rows for a batch of n: the three edge rows (every column 0, 1/2, the largest fp32 below 1), rows mixing the edges
    column by column (both translation extremes, the cut clipped at each border, in one row), and random rows; cut into batches
    of n (the last one wraps)."""
    rng = np.random.RandomState(seed)
    pool = [np.full(8, e, np.float32) for e in EDGE_U]
    lo, hi = EDGE_U[0], EDGE_U[2]
    pool.append(np.array([0.3, 0.9, 0.1, lo, hi, hi, lo, 0.0], np.float32))
    pool.append(np.array([0.7, 0.2, 0.8, hi, lo, lo, hi, 0.0], np.float32))
    pool += [rng.uniform(0, 1, 8).astype(np.float32) for _ in range(max(3, n))]
    pool = np.minimum(np.stack(pool), np.float32(hi))
    batches = []
    for r in range(0, len(pool), n):
        batches.append(np.stack([pool[(r + k) % len(pool)] for k in range(n)]))
    return batches


def images(shape, seed):
    """fp32 test batch: noise in [-1, 1]; where the batch has them, sample 1 is 1000 + noise and sample 2 all zeros."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    if shape[0] > 1:
        x[1] += np.float32(1000)
    if shape[0] > 2:
        x[2] = 0
    return x


def bound(x):
    """The a priori forward bound per sample, [n, 1, 1, 1]: 64 * 2^-24 * (max |x| of the sample + 1) -- at most ten roundings, each of
    a quantity no larger than 6 (max |x| + 1/2).  The transpose's bound has max |dy| in the place of max |x| + 1 (bound(dy, 0))."""
    return bound_of(x, 1.0)


def bound_of(x, plus):
    a = np.abs(np.asarray(x, np.float64)).reshape(x.shape[0], -1).max(axis=1) + plus
    return (64 * 2.0 ** -24 * a).reshape(-1, 1, 1, 1)
