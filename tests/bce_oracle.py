"""The four formulas of csrc/sigmoid_xent.hip stated on the CPU (NumPy), in fp64 or np.longdouble from the fp32 inputs and NOT
rounded to fp32: torch.nn.functional.binary_cross_entropy_with_logits(reduction='none', pos_weight=w) with the ignored-target
rule, its gradient in the two one-sided forms, the statistics of igan_sigmoid_xent_stats_update, and the probability pairs of
igan_binary_probs.  Also the inputs of tests/test_gpu_sigmoid_xent.py, so that every test draws the same matrices."""
import numpy as np

SHAPES = ((1, 1), (3, 40), (257, 40), (64, 64), (1031, 5))      # a single element, the metric's width, a grid tail, an exact
#                                                                  wave multiple, odd rows with only 4-byte alignment
FLT_MAX = float(np.finfo(np.float32).max)
PLANTED = (0.0, 1e-30, 1e-38, 1e-45, 17.0, 88.0, 104.0, 1e4, FLT_MAX)      # each with both signs; 1e-38 and 1e-45 are fp32 denormals


def logits_of(n, A, seed):
    """Seeded normal x 8 with the planted magnitudes written over the head of the matrix, each as +v, -v, +v, -v (as many as fit):
    targets_of gives the four copies the targets 0, 0, 1, 1, so that both signs meet both classes."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(n, A) * 8).astype(np.float32)
    planted = np.array([s * v for v in PLANTED for s in (1.0, -1.0, 1.0, -1.0)], dtype=np.float32)
    flat = x.reshape(-1)
    k = min(planted.size, flat.size - 1)       # the last element stays a draw: (1, 1) is the seeded normal alone
    flat[:k] = planted[:k]
    return x


def targets_of(n, A, seed):
    """A mix of 0, 1, -1 and NaN (about 40 / 40 / 10 / 10 %); the planted head of logits_of gets 0, 0, 1, 1 repeated."""
    rng = np.random.RandomState(seed + 1000)
    t = rng.choice(np.array([0.0, 1.0, -1.0, np.nan], dtype=np.float32), size=(n, A), p=[0.4, 0.4, 0.1, 0.1]).astype(np.float32)
    flat = t.reshape(-1)
    k = min(4 * len(PLANTED), flat.size - 1)
    flat[:k] = ((np.arange(k) // 2) % 2).astype(np.float32)
    return t


def pos_weight_of(A, seed):
    return (0.25 + 4.0 * np.random.RandomState(seed + 2000).rand(A)).astype(np.float32)


def kinds(t):
    """(positive, negative) masks: t == 1, t == 0; everything else (NaN and -1 included) is ignored."""
    t = np.asarray(t)
    with np.errstate(invalid='ignore'):
        return t == 1.0, t == 0.0


def softplus(z):
    """max(z, 0) + log1p(exp(-|z|)) in the precision of z; the max as a comparison, so that a NaN stays a NaN."""
    with np.errstate(all='ignore'):
        return np.where(z > 0, z, np.zeros_like(z)) + np.log1p(np.exp(-np.abs(z)))


def _weights(x, pos_weight, dtype):
    w = np.ones(x.shape[1], dtype) if pos_weight is None else np.asarray(pos_weight).astype(dtype)
    return np.broadcast_to(w[None, :], x.shape)


def forward(x, t, pos_weight=None, dtype=np.longdouble):
    """(loss [n, A] in `dtype`, pred [n, A] int8) of fp32 logits x against fp32 targets t."""
    z = np.asarray(x).astype(dtype)
    pos, neg = kinds(t)
    with np.errstate(all='ignore'):
        loss = np.where(pos, _weights(z, pos_weight, dtype) * softplus(-z), np.where(neg, softplus(z), np.zeros_like(z)))
        pred = (np.asarray(x) > 0).astype(np.int8)
    return loss, pred


def backward(x, t, dloss, pos_weight=None, dtype=np.longdouble):
    """dlogits [n, A] in `dtype`: dloss * (-w / (1 + exp(x))) at a positive, dloss * (1 / (1 + exp(-x))) at a negative, 0 elsewhere."""
    z = np.asarray(x).astype(dtype)
    pos, neg = kinds(t)
    one = dtype(1)
    with np.errstate(all='ignore'):
        g_pos = -_weights(z, pos_weight, dtype) / (one + np.exp(z))
        g_neg = one / (one + np.exp(-z))
        return np.where(pos, np.asarray(dloss).astype(dtype) * g_pos, np.where(neg, np.asarray(dloss).astype(dtype) * g_neg, np.zeros_like(z)))


def binary_probs(x, dtype=np.longdouble):
    """probs [A, n, 2] in `dtype`: softmax of the pair (x, -x), attribute-major: (1 / (1 + exp(-2x)), 1 / (1 + exp(2x)))."""
    z2 = 2 * np.asarray(x).astype(dtype).T
    one = dtype(1)
    with np.errstate(all='ignore'):
        return np.stack([one / (one + np.exp(-z2)), one / (one + np.exp(z2))], axis=-1)


def stats(loss, x, t):
    """(loss_sum [A] fp64, counts [A, 4] int64: tp, fp, tn, fn) of fp32 losses: every column summed serially in row order with
    one fp64 accumulator, ignored elements neither added nor counted."""
    loss, x = np.asarray(loss), np.asarray(x)
    pos, neg = kinds(t)
    n, A = x.shape
    total = np.zeros(A, np.float64)
    with np.errstate(all='ignore'):
        for r in range(n):
            total = np.where(pos[r] | neg[r], total + loss[r].astype(np.float64), total)
        p = x > 0
    counts = np.stack([(pos & p).sum(0), (neg & p).sum(0), (neg & ~p).sum(0), (pos & ~p).sum(0)], axis=1).astype(np.int64)
    return total, counts


def half_spacing_bound(ref):
    """0.5 * spacing_fp32(ref) * (1 + 2^-20), elementwise in fp64: what one rounding of an fp64 value to fp32 may cost, with
    room for the few-fp64-ulp error of the device's exp / log1p.  Where ref is infinite or NaN the bound is 0 and the caller
    compares exactly."""
    with np.errstate(all='ignore'):
        r32 = np.abs(np.asarray(ref).astype(np.float32))
        sp = np.spacing(r32).astype(np.float64)
        sp = np.where(np.isfinite(sp), sp, 2.0 ** 104)        # at the largest finite fp32 there is no next value: its binade's spacing
        return np.where(np.isfinite(r32), 0.5 * sp * (1 + 2.0 ** -20), 0.0)


def within_half_spacing(got, ref):
    """(ok, worst ratio): every fp32 `got` is within half_spacing_bound of the unrounded `ref`; an infinite reference (after
    rounding to fp32) must be met exactly and a NaN by a NaN."""
    got64 = np.asarray(got).astype(np.longdouble)
    ref = np.asarray(ref)
    with np.errstate(all='ignore'):
        ref32 = ref.astype(np.float32)
        finite = np.isfinite(ref32)
        bound = half_spacing_bound(ref)
        err = np.abs(got64 - ref.astype(np.longdouble)).astype(np.float64)
        same_special = np.where(np.isnan(ref32), np.isnan(np.asarray(got)), np.asarray(got) == ref32)
        ok = np.where(finite, err <= bound, same_special)
        ratio = np.where(finite, err / np.where(bound > 0, bound, 1.0), 0.0)
    return bool(np.all(ok)), float(np.max(ratio, initial=0.0))
