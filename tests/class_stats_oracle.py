"""fp64 NumPy oracle of csrc/class_stats.hip and of what hip_ops.ClassHistogram / SplitProbStats build on it, with the inputs
the tests share.  Everything here is the plain statement: np.argmax / np.bincount for the histogram, fp64 sums of the float32
probabilities for psum / plogp, and the reference's Inception Score statement (metrics/inception_score.py:50-54) evaluated
in fp64 for a split's score."""
import numpy as np

NS = (1, 3, 65, 257)
KS = (1, 2, 63, 64, 65, 1000, 1001)


def logit_rows(n, K, seed):
    """float32 logits with many exact ties: values on a coarse grid, so that equal maxima are the rule and not the exception."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-6, 7, size=(n, K)) * 0.25).astype(np.float32)


def crafted_rows(K):
    """Rows of width K >= 130 that pin np.argmax's tie and NaN rules; -> float32 [rows, K]."""
    assert K >= 130
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    rows = []

    def row(fill=-1.0, **at):
        r = np.full(K, fill, dtype=np.float32)
        for k, v in at.items():
            r[int(k[1:])] = v
        rows.append(r)

    row(c70=2.0, c6=2.0)                            # equal maxima 64 columns apart: one lane holds both
    row(c71=2.0, c7=2.0, c129=2.0)
    row(c9=3.0, c10=3.0, c11=3.0)                   # inside one 4-wide group
    row(c66=3.0, c65=3.0)
    row(c100=3.0, c37=3.0)                          # in different lanes: the wave reduction breaks the tie
    row(fill=-2.0, c5=-0.0, c3=0.0)                 # -0.0 == +0.0: the lower index
    row(fill=-2.0, c3=-0.0, c5=0.0)
    row(fill=-2.0, c64=-0.0, c0=0.0)
    row(c80=inf, c17=inf)                           # +inf ties
    row(c17=inf, c16=inf)
    row(fill=-inf)                                  # all -inf: 0
    row(fill=-inf, c129=-3.0e38)
    row(c77=nan, c3=5.0)                            # one NaN
    row(c3=nan, c77=nan)                            # two NaNs: the first
    row(c77=nan, c78=nan)
    row(c4=inf, c90=nan)                            # a NaN after a +inf
    row(c90=nan, c91=inf)
    row(c0=nan, c64=nan, c128=nan)
    row(fill=nan)
    r = np.full(K, 1.0, dtype=np.float32)           # all equal
    rows.append(r)
    tail = np.full(K, -1.0, dtype=np.float32)       # the maximum in the last, ungrouped columns
    tail[K - 1] = 4.0
    rows.append(tail)
    return np.stack(rows)


def argmax_hist(x):
    labels = np.argmax(x, axis=1)
    return labels, np.bincount(labels, minlength=x.shape[1])


def softmax_rows(n, K, seed, scale=3.0):
    """float32 probability rows with no zero (the softmax of logits within +- 3 scale)."""
    rng = np.random.RandomState(seed)
    z = rng.randn(n, K) * scale
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    assert (p > 0).all()
    return p


def prob_sums(p):
    """(psum [K], plogp) of float32 rows, fp64."""
    d = np.asarray(p, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return d.sum(axis=0), float(np.sum(d * np.log(d)))


def split_bounds(num_images, num_splits):
    return [(i * num_images // num_splits, (i + 1) * num_images // num_splits) for i in range(num_splits)]


def split_scores(p, num_splits):
    """The reference's statement over the splits of the float32 rows p [N, K], every operation in fp64."""
    d = np.asarray(p, dtype=np.float64)
    scores = []
    with np.errstate(divide='ignore', invalid='ignore'):
        for b, e in split_bounds(d.shape[0], num_splits):
            part = d[b:e]
            kl = part * (np.log(part) - np.log(np.expand_dims(np.mean(part, 0), 0)))
            scores.append(np.exp(np.mean(np.sum(kl, 1))))
    return np.asarray(scores)


def split_sums(p, num_splits):
    """(n [S], psum [S, K], plogp [S]) of the splits, fp64."""
    sums = [prob_sums(p[b:e]) for b, e in split_bounds(p.shape[0], num_splits)]
    n = np.array([e - b for b, e in split_bounds(p.shape[0], num_splits)], dtype=np.float64)
    return n, np.stack([s[0] for s in sums]), np.array([s[1] for s in sums])


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), np.finfo(np.float64).tiny)))
