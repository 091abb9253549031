"""fp64 restatement of csrc/softmax_xent.hip on the CPU (NumPy): torch.nn.functional.cross_entropy(reduction='none') as
include/igan_hip.h states it, with the ignored-row rule, np.argmax, and the sums of igan_xent_stats_update.  Also the input
families of tests/test_gpu_softmax_xent.py, so that every test draws the same rows."""
import numpy as np

KS = (1, 2, 3, 10, 63, 64, 65, 257, 1000)
NS = (1, 5, 17, 192)
KINDS = ('normal', 'scaled90', 'equal', 'neginf')


def logits_of(kind, n, K, seed):
    rng = np.random.RandomState(seed)
    x = rng.randn(n, K).astype(np.float32)
    if kind == 'scaled90':                      # exp overflows fp32 (e^89) without the max shift
        x = (x / np.abs(x).max() * 90.0).astype(np.float32)
    elif kind == 'equal':                       # every row one value: lse = v + log K, arg-max 0
        x = np.repeat(rng.randn(n, 1).astype(np.float32), K, axis=1)
    elif kind == 'neginf':                      # one -inf column per row (K = 1: the row of -inf, a NaN row)
        x[np.arange(n), rng.randint(K, size=n)] = -np.inf
    return x


def labels_of(n, K, seed):
    """Valid labels with -1 and K (both ignored) sprinkled in; row 0 keeps a valid label."""
    rng = np.random.RandomState(seed + 77)
    lab = rng.randint(K, size=n).astype(np.int32)
    if n >= 5:
        lab[1::7] = -1
        lab[3::11] = K
    return lab


def _lse(x, parts=False):
    """m + log1p(sum over k != argmax of exp(x_k - m)) in the precision of x: the arg-max column's term of the sum is exactly 1.
    That column contributes x - m itself -- 0 for a finite maximum, NaN for a maximum of +-inf or NaN (np.max gives NaN for a row
    that holds one), which is what makes such a row NaN."""
    n = x.shape[0]
    best = np.argmax(x, axis=1)
    m = np.max(x, axis=1)
    a = x - m[:, None]
    terms = np.exp(a)
    terms[np.arange(n), best] = a[np.arange(n), best]
    logs = np.log1p(np.sum(terms, axis=1))
    return (m + logs, m, logs) if parts else m + logs


def forward(x, labels):
    """(loss [n] fp32, lse [n] fp64, pred [n]) of x [n, K] fp32."""
    x64 = x.astype(np.float64)
    n, K = x.shape
    with np.errstate(all='ignore'):
        lse = _lse(x64)
        valid = (labels >= 0) & (labels < K)
        picked = x64[np.arange(n), np.where(valid, labels, 0)]
        loss = np.where(valid, lse - picked, 0.0).astype(np.float32)
    return loss, lse, np.argmax(x, axis=1).astype(np.int32)


def lse_reference(x):
    """(lse, bound, cancelling) per row: lse = m + log S evaluated in np.longdouble (64-bit significand: its own error is
    2^-11 of an fp64 spacing; as
    the kernel, with log1p of the sum without the arg-max column) and rounded to fp64 only for the comparison, and the absolute error allowed to the kernel.

    A row CANCELS when |lse| < max(|m|, |log S|) / 2: the addition m + log S loses at least one bit, and errors made at the
    size of log S no longer shrink with the result.  Elsewhere the bound is 4 fp64 spacings at |lse|.  On a cancelling row it
    is the sum of what the arithmetic of include/igan_hip.h can do, with u = 2^-53:
        S        every exp is good to an ulp (2 u relative), each of the D additions on the longest path to the sum rounds
                 once (u relative, all terms positive), x - m is exact or rounds once: (D + 3) u relative, which is the same
                 ABSOLUTE error in log S;  D = 4 ceil((K / 4) / 64) + 1 + 6 (a lane's columns, its tail column, the six
                 steps of the lane tree);
        log      an ulp: one spacing at |log S|;
        m + .    half a spacing at |lse|."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, 'np.longdouble is not wider than fp64 on this machine'
    xl = x.astype(np.longdouble)
    K = x.shape[1]
    with np.errstate(all='ignore'):
        lse, m, logs = _lse(xl, parts=True)
        lse64, m64, logs64 = lse.astype(np.float64), np.abs(m).astype(np.float64), np.abs(logs).astype(np.float64)
        cancelling = np.abs(lse64) < np.maximum(m64, logs64) / 2
        depth = 4 * -(-(K // 4) // 64) + 1 + 6
        derived = 0.5 * np.spacing(np.abs(lse64)) + np.spacing(logs64) + (depth + 3) * 2.0 ** -53
        bound = np.where(cancelling, derived, 4 * np.spacing(np.abs(lse64)))
    return lse, bound, cancelling


def backward(x, labels, lse, dloss):
    """dlogits [n, K] in fp64 (not rounded), from the lse handed in."""
    n, K = x.shape
    valid = (labels >= 0) & (labels < K)
    with np.errstate(all='ignore'):
        a = x.astype(np.float64) - lse[:, None]
        onehot = np.zeros((n, K), dtype=bool)
        onehot[np.arange(n)[valid], labels[valid]] = True
        d = dloss.astype(np.float64)[:, None] * np.where(onehot, np.expm1(a), np.exp(a))     # p - 1 without the cancellation
    d[~valid] = 0.0
    return d


def stats(loss, labels, pred, K):
    """(sum of loss in fp64 in row order, rows counted, rows correct) over the rows with a label in [0, K)."""
    total, counted, correct = 0.0, 0, 0
    for l, t, p in zip(loss, labels, pred):
        if 0 <= t < K:
            total += float(l)
            counted += 1
            correct += int(p == t)
    return total, counted, correct


def ulps32(got, want):
    """|got - want| in units of the fp32 spacing at want (the oracle value rounded to fp32), elementwise.
    An infinity (the loss of a label at a -inf column) must be met exactly."""
    with np.errstate(all='ignore'):
        want32 = np.asarray(want).astype(np.float32)
        got64 = np.asarray(got, np.float64)
        u = np.abs(got64 - np.asarray(want, np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
        return np.where(np.isinf(want32), np.where(got64 == want32, 0.0, np.inf), u)


def ulps64(got, want, scale=None):
    """|got - want| in fp64 spacings at |want|, or at `scale` when given."""
    with np.errstate(all='ignore'):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        at = np.abs(want) if scale is None else np.asarray(scale, np.float64)
        return np.where(np.isinf(want), np.where(got == want, 0.0, np.inf), np.abs(got - want) / np.spacing(at))
