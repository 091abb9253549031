"""The small dense kernels (csrc/dense_small.hip) restated in fp64 from include/igan_hip.h -- the comment blocks of igan_dense_params,
igan_dense2_params, the two weight-gradient structs, igan_rows_group_sum and the taps entry points -- with the case tables, the input
generator and the guard-band arena shared by tests/test_dense_cases.py (host) and tests/test_gpu_dense_small.py.  NumPy only: no
device is needed to import it.

Inputs are fp32 values; every reference widens them to double first, so a reference differs from a kernel by the kernel's own
rounding only.  A tensor is seeded by its name, its form and its shape.  Values lean positive (randn + 0.5) so that a single output
element -- N = 1, M = 1 are cases -- is not a cancelled sum whose relative error means nothing; the last k-quad of a dense operand and
the last row of a weight-gradient operand are "loud" (positive, magnitude in [1, 2)), so that a kernel that loses exactly that
quad or row moves every output by a known share.  These are conditions on the inputs, held by tests/test_dense_cases.py with an fp32
model of the kernel's summation and a list of mutants of the restatement; they are never fitted to what a kernel returns."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

PRO_NONE, PRO_SQUARE, PRO_DEMOD_GRAD, PRO_MUL = 0, 1, 2, 3
EPI_SCALE, EPI_BIAS, EPI_RSQRT, EPI_STYLE_GRAD, EPI_DEMOD_GRAD2, EPI_STYLE_GRAD2 = 0, 1, 2, 3, 4, 5
MAX_GROUPS = 24

SENTINEL = np.float32(-24680.25)      # finite, exact in fp32, far from every O(1) result: guard bands and unwritten outputs hold it
GUARD = 64                            # floats between any two tensors of an arena

# scalars: none is 0 or 1, so a dropped factor shows
_f = lambda v: float(np.float32(v))      # the fp32 value the struct carries, widened
ALPHA, BIAS_SCALE, ADD_CONST, EPS = _f(0.7), _f(1.3), 0.75, 0.0625
PRO_SCALE = {PRO_NONE: _f(0.45), PRO_SQUARE: _f(0.45), PRO_DEMOD_GRAD: _f(-0.35), PRO_MUL: _f(1.9)}      # NONE / SQUARE must ignore theirs
ALPHA2 = _f(-0.6)
TAPS_SCALE = _f(1.7)

# the bounds of the issue's table (tests.util.rel_err against the fp64 restatement)
BOUND_SCALE, BOUND_FWD, BOUND_GRAD, BOUND_SECOND = 3e-5, 1e-5, 2e-5, 1e-4


# ----------------------------------------------------------------------------- fp64 restatement
def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def prologue64(x, prologue, x2=None, pro_scale=0.0):
    x, x2 = _f64(x), _f64(x2)
    if prologue == PRO_SQUARE:
        return x * x
    if prologue == PRO_DEMOD_GRAD:
        return pro_scale * x * x2 ** 3
    if prologue == PRO_MUL:
        return pro_scale * x * x2
    assert prologue == PRO_NONE
    return x


def dense(x, w, *, wt=False, alpha=1.0, prologue=PRO_NONE, x2=None, pro_scale=0.0, epilogue=EPI_SCALE, bias=None, bias_scale=1.0,
          add_const=0.0, eps=0.0, e1=None, e2=None, e3=None, want_y2=False, want_colsum=False):
    """y = epi(alpha * pro(x) . W), W = w[k][n] or w[n][k] when wt.  -> dict(y=[M, N]) plus y2 [M, N] (the bare product beside every
    epilogue but DEMOD_GRAD2, whose y2 is 3/4 v e1 e2^5) and colsum [N] = bias_scale * sum_m y[m, n] where asked."""
    W = _f64(w).T if wt else _f64(w)
    v = alpha * (prologue64(x, prologue, x2, pro_scale) @ W)
    bias, e1, e2, e3 = _f64(bias), _f64(e1), _f64(e2), _f64(e3)
    y2 = v
    if epilogue == EPI_SCALE:
        y = v
    elif epilogue == EPI_BIAS:
        y = v + bias_scale * bias[None, :] + add_const
    elif epilogue == EPI_RSQRT:
        y = 1.0 / np.sqrt(v + eps)
    elif epilogue == EPI_STYLE_GRAD:
        y = 2.0 * e2 * v + (e1 if e1 is not None else 0.0)
    elif epilogue == EPI_DEMOD_GRAD2:
        y = -0.5 * v * e2 ** 3
        y2 = 0.75 * v * e1 * e2 ** 5
    else:
        assert epilogue == EPI_STYLE_GRAD2
        y = 2.0 * (e2 * v + e1 * e3)
    out = dict(y=y)
    if want_y2 or epilogue == EPI_DEMOD_GRAD2:
        out['y2'] = y2
    if want_colsum:
        out['colsum'] = bias_scale * y.sum(axis=0)
    return out


def wgrad(a, b, *, alpha=1.0, pro_a=PRO_NONE, pro_b=PRO_NONE, b2=None, pro_scale=0.0):
    """dw[k, n] = alpha * sum_m pro_a(a)[m, k] * pro_b(b)[m, n]   (pro_a NONE | SQUARE, pro_b NONE | DEMOD_GRAD with b2)."""
    return alpha * (prologue64(a, pro_a).T @ prologue64(b, pro_b, b2, pro_scale))


def wgrad2(a, a2, b, b2, c, d, *, alpha=1.0, alpha2=0.0, pro_b=PRO_NONE, pro_c=PRO_NONE, pro_scale=0.0):
    """dw[k, n] = alpha * sum_m a a2 pro_b(b) + alpha2 * sum_m pro_c(c) d   (a2 None = 1; c None = no second term)."""
    aa = _f64(a) * (_f64(a2) if a2 is not None else 1.0)
    dw = alpha * (aa.T @ prologue64(b, pro_b, b2, pro_scale))
    if c is not None:
        dw = dw + alpha2 * (prologue64(c, pro_c).T @ _f64(d))
    return dw


def sumsq_taps(w):
    """w [taps, n] -> out[i] = sum_t w[t, i]^2."""
    w = _f64(w)
    return (w * w).sum(axis=0)


def bcast_mul_taps(w, v, scale):
    """out[t, i] = scale * w[t, i] * v[i]."""
    return scale * _f64(w) * _f64(v)[None, :]


def rows_group_sum(src, slots, L):
    """out[m, j, :] = sum over the groups l with slots[l] == j, IN ORDER and in fp32 (the header promises the order: the GPU test
    compares bit for bit), of src[l, m, :]; zero where no group names j."""
    src = np.asarray(src, np.float32)
    out = np.zeros((src.shape[1], L, src.shape[2]), np.float32)
    for l, j in enumerate(slots):
        out[:, j, :] = out[:, j, :] + src[l]
    return out


# ----------------------------------------------------------------------------- inputs
def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _lean(rng, shape, scale=1.0):
    return ((rng.standard_normal(shape) + 0.5) * scale).astype(np.float32)


def _unit(rng, shape):
    return rng.uniform(0.5, 1.5, size=shape).astype(np.float32)


def _loud(v):
    """Positive, magnitude in [1, 2)."""
    return (1.0 + np.abs(v) % 1.0).astype(np.float32)


# name: prologue, epilogue, colsum, e1 present, y2 asked, entry point (1 = igan_dense_small[_grouped], 2 = igan_dense_small2_grouped),
# bound of y.  y2 is held to BOUND_SECOND, colsum to BOUND_GRAD beside STYLE_GRAD and to BOUND_SECOND beside STYLE_GRAD2.
FORMS = {
    'scale': (PRO_NONE, EPI_SCALE, False, False, False, 1, BOUND_SCALE),
    'bias': (PRO_NONE, EPI_BIAS, False, False, False, 1, BOUND_FWD),
    'rsqrt': (PRO_SQUARE, EPI_RSQRT, False, False, False, 1, BOUND_FWD),
    'style_grad': (PRO_DEMOD_GRAD, EPI_STYLE_GRAD, True, True, False, 1, BOUND_GRAD),
    'style_grad_no_e1': (PRO_DEMOD_GRAD, EPI_STYLE_GRAD, True, False, False, 1, BOUND_GRAD),
    'mul_y2': (PRO_MUL, EPI_SCALE, False, False, True, 2, BOUND_SECOND),
    'bias_y2': (PRO_NONE, EPI_BIAS, False, False, True, 2, BOUND_FWD),
    'demod_grad2': (PRO_NONE, EPI_DEMOD_GRAD2, False, True, False, 2, BOUND_SECOND),
    'style_grad2': (PRO_NONE, EPI_STYLE_GRAD2, True, True, False, 2, BOUND_SECOND),
}
EDGE_FORMS = ('style_grad', 'style_grad_no_e1')      # these also run the bucket edges
MS, MS_EDGES = (1, 9, 24, 33, 64), (8, 16, 17, 25, 32, 48, 49)
KS, NS = (4, 260, 516), (1, 5, 8)


def dense_shapes(form):
    """(M, K, N, ldx, ldy) of the single-launch tests: ldx = 3 K is the [:, 1] slice of an [M, 3, K] tensor."""
    ms = MS + (MS_EDGES if form in EDGE_FORMS else ())
    return [(M, K, N, ldx, ldy) for M in ms for K in KS for N in NS for ldx in (K, 3 * K) for ldy in (N, N + 3)]


def bounds(form):
    _, epi, _, _, _, _, by = FORMS[form]
    return dict(y=by, y2=BOUND_SECOND, colsum=BOUND_SECOND if epi == EPI_STYLE_GRAD2 else BOUND_GRAD)


@functools.lru_cache(maxsize=None)
def dense_case(form, wt, M, K, N, ldx=None, ldy=None):
    """One problem: fp32 operands as the kernel reads them (x_full [M, ldx] with x its columns xoff .. xoff + K; w in its stored
    layout), the scalars, and the fp64 reference `ref`.  Cached and shared: never written to."""
    pro, epi, colsum, has_e1, want_y2, entry, _ = FORMS[form]
    ldx, ldy = ldx or K, ldy or N
    assert K % 4 == 0 and ldx in (K, 3 * K) and ldy >= N
    key = (form, wt, M, K, N, ldx)
    x_full = _lean(_rng('x', *key), (M, ldx))
    xoff = K if ldx == 3 * K else 0
    x_full[:, xoff + K - 4:xoff + K] = _loud(x_full[:, xoff + K - 4:xoff + K])
    x = x_full[:, xoff:xoff + K]
    x2 = None
    if pro == PRO_DEMOD_GRAD:
        x2 = _unit(_rng('x2', *key), (M, K))
    elif pro == PRO_MUL:
        x2 = _lean(_rng('x2', *key), (M, K))
        x2[:, K - 4:] = _loud(x2[:, K - 4:])
    r = _rng('w', *key)
    if epi == EPI_RSQRT:        # a sum of squares, like sum_taps(w^2): v + eps > 0
        W = (r.standard_normal((3, K, N)) ** 2).mean(axis=0)
        W[K - 4:] = _loud(W[K - 4:])
        W = (W / K).astype(np.float32)
    else:
        W = r.standard_normal((K, N)) + 0.5
        W[K - 4:] = _loud(W[K - 4:])
        W = (W / (0.25 * K + np.sqrt(K))).astype(np.float32)
    c = SimpleNamespace(form=form, wt=bool(wt), M=M, K=K, N=N, ldx=ldx, ldy=ldy, xoff=xoff, prologue=pro, epilogue=epi, entry=entry,
                        x_full=x_full, x=x, x2=x2, W=W, w=np.ascontiguousarray(W.T) if wt else W,
                        bias=_lean(_rng('bias', *key), (N,), 0.5) if epi == EPI_BIAS else None,
                        # e1 leans the way of the term it is added to (pro_scale < 0 turns DEMOD_GRAD's product negative)
                        # and stays away from zero where it is a factor (STYLE_GRAD2's e1 e3, with e3)
                        e1=None if not has_e1 else _unit(_rng('e1', *key), (M, N)) if epi == EPI_STYLE_GRAD2 else
                        _lean(_rng('e1', *key), (M, N), -0.5 if pro == PRO_DEMOD_GRAD else 0.5),
                        e2=_unit(_rng('e2', *key), (M, N)) if epi in (EPI_STYLE_GRAD, EPI_DEMOD_GRAD2, EPI_STYLE_GRAD2) else None,
                        e3=_unit(_rng('e3', *key), (M, N)) if epi == EPI_STYLE_GRAD2 else None,
                        alpha=ALPHA, pro_scale=PRO_SCALE[pro], bias_scale=BIAS_SCALE, add_const=ADD_CONST, eps=EPS,
                        want_y2=want_y2 or epi == EPI_DEMOD_GRAD2, want_colsum=colsum)
    c.ref = dense_of(c)
    for a in (c.x_full, c.x2, c.W, c.w, c.bias, c.e1, c.e2, c.e3) + tuple(c.ref.values()):
        if a is not None:
            a.setflags(write=False)
    return c


def dense_of(c, **over):
    """dense() on a case's operands; `over` replaces arguments (the mutants of test_dense_cases.py)."""
    kw = dict(x=c.x, w=c.w, wt=c.wt, alpha=c.alpha, prologue=c.prologue, x2=c.x2, pro_scale=c.pro_scale, epilogue=c.epilogue, bias=c.bias,
              bias_scale=c.bias_scale, add_const=c.add_const, eps=c.eps, e1=c.e1, e2=c.e2, e3=c.e3, want_y2=c.want_y2, want_colsum=c.want_colsum)
    kw.update(over)
    x, w = kw.pop('x'), kw.pop('w')
    return dense(x, w, **kw)


# grouped launches: (form, M, K, N) per group, all (M, K, N) different, groups on both sides of every bucket edge (8 | 16 | 24 | 32 | 48)
GROUPED_BIAS = [('bias', M, K, N) for M, K, N in [
    (1, 4, 1), (64, 516, 10), (8, 260, 5), (9, 8, 3), (16, 516, 1), (17, 128, 8), (24, 4, 7), (25, 260, 12), (32, 512, 2), (33, 256, 5),
    (48, 260, 9), (49, 516, 4), (3, 516, 6), (12, 12, 11), (20, 264, 1), (28, 1028, 3), (40, 4, 13), (56, 520, 2), (2, 260, 1), (5, 16, 8),
    (7, 772, 5), (60, 4, 4), (63, 260, 7), (64, 8, 1)]]
GROUPED_STYLE = [('style_grad', 3, 260, 5), ('style_grad_no_e1', 33, 516, 1), ('style_grad', 17, 4, 8), ('style_grad', 48, 260, 10),
                 ('style_grad_no_e1', 9, 12, 3)]
GROUPED_SECOND = [('mul_y2', 9, 260, 5), ('bias_y2', 49, 4, 1), ('demod_grad2', 24, 516, 8), ('style_grad2', 1, 8, 10)]
assert len(GROUPED_BIAS) == MAX_GROUPS == len(set(g[1:] for g in GROUPED_BIAS))


def grouped_cases(table, wt):
    """The problems of one grouped launch; group i is padded to ldy = N + (i % 2) * 3 and sliced out of [M, 3, K] when i % 3 == 1."""
    return [dense_case(form, wt, M, K, N, 3 * K if i % 3 == 1 else K, N + 3 * (i % 2)) for i, (form, M, K, N) in enumerate(table)]


# ----------------------------------------------------------------------------- weight gradients
WGRAD_MS = (1, 7, 8, 9, 33, 64)
WGRAD_KN = ((1, 4), (5, 260), (260, 12))      # (5, 260): 325 threads, a ragged second block


def wgrad_shapes():
    return [(M, K, N, lda) for M in WGRAD_MS for K, N in WGRAD_KN for lda in (K, 3 * K)]


def _wg_operand(name, key, M, K, ld, loud=True):
    full = _lean(_rng(name, *key), (M, ld))
    off = K if ld == 3 * K else 0
    if loud:
        full[M - 1, off:off + K] = _loud(full[M - 1, off:off + K])
    return full, off


@functools.lru_cache(maxsize=None)
def wgrad_case(M, K, N, lda, pro_a, pro_b):
    key = (M, K, N, lda, pro_a, pro_b)
    a_full, aoff = _wg_operand('wg.a', key, M, K, lda)
    b = _lean(_rng('wg.b', *key), (M, N))
    b[M - 1] = _loud(b[M - 1])
    c = SimpleNamespace(M=M, K=K, N=N, lda=lda, aoff=aoff, a_full=a_full, a=a_full[:, aoff:aoff + K], b=b,
                        b2=_unit(_rng('wg.b2', *key), (M, N)) if pro_b == PRO_DEMOD_GRAD else None, pro_a=pro_a, pro_b=pro_b,
                        alpha=float(np.float32(ALPHA / np.sqrt(M))), pro_scale=PRO_SCALE[pro_b])
    c.ref = wgrad_of(c)
    return c


def wgrad_of(c, rows=None):
    """wgrad() on a case; rows = the row count a mutant sums."""
    r = slice(0, c.M if rows is None else rows)
    return wgrad(c.a[r], c.b[r], alpha=c.alpha, pro_a=c.pro_a, pro_b=c.pro_b, b2=None if c.b2 is None else c.b2[r], pro_scale=c.pro_scale)


def wgrad_forms():
    return [(pa, pb) for pa in (PRO_NONE, PRO_SQUARE) for pb in (PRO_NONE, PRO_DEMOD_GRAD)]


def wgrad2_forms():
    """(a2 present, pro_b, c: None = absent | pro_c)."""
    return [(a2, pb, pc) for a2 in (False, True) for pb in (PRO_NONE, PRO_DEMOD_GRAD) for pc in (None, PRO_NONE, PRO_SQUARE)]


@functools.lru_cache(maxsize=None)
def wgrad2_case(M, K, N, lda, ldc, has_a2, pro_b, pro_c):
    key = (M, K, N, lda, ldc, has_a2, pro_b, pro_c)
    a_full, aoff = _wg_operand('wg2.a', key, M, K, lda)
    b = _lean(_rng('wg2.b', *key), (M, N))
    b[M - 1] = _loud(b[M - 1])
    c = SimpleNamespace(M=M, K=K, N=N, lda=lda, ldc=ldc, aoff=aoff, a_full=a_full, a=a_full[:, aoff:aoff + K], b=b, a2=None, c_full=None, c=None,
                        coff=0, d=None, b2=_unit(_rng('wg2.b2', *key), (M, N)) if pro_b == PRO_DEMOD_GRAD else None, pro_b=pro_b,
                        pro_c=pro_c if pro_c is not None else PRO_NONE, alpha=float(np.float32(ALPHA / np.sqrt(M))),
                        alpha2=float(np.float32(ALPHA2 / np.sqrt(M))), pro_scale=PRO_SCALE[pro_b])
    if has_a2:
        c.a2 = _lean(_rng('wg2.a2', *key), (M, K))
        c.a2[M - 1] = _loud(c.a2[M - 1])
    if pro_c is not None:
        c.c_full, c.coff = _wg_operand('wg2.c', key, M, K, ldc)
        c.c = c.c_full[:, c.coff:c.coff + K]
        c.d = _lean(_rng('wg2.d', *key), (M, N))
        c.d[M - 1] = -_loud(c.d[M - 1])      # with alpha2 < 0 the second term's last row adds to the first's
    c.ref = wgrad2_of(c)
    return c


def wgrad2_of(c, rows=None):
    r = slice(0, c.M if rows is None else rows)
    cut = lambda t: None if t is None else t[r]
    return wgrad2(c.a[r], cut(c.a2), c.b[r], cut(c.b2), cut(c.c), cut(c.d), alpha=c.alpha, alpha2=c.alpha2, pro_b=c.pro_b, pro_c=c.pro_c,
                  pro_scale=c.pro_scale)


WGRAD_GROUPED = [(9, 1, 4), (64, 5, 260), (7, 260, 12), (33, 3, 8), (1, 64, 4), (8, 130, 8)]      # (M, K, N): six different K * N


# ----------------------------------------------------------------------------- taps, rows_group_sum
TAPS_SHAPES = [(t, n) for t in (1, 9) for n in (4, 1028)]      # n = 1028: 257 lanes, one in a second block
TAPS_GROUPED = [(1, 4), (9, 1028), (3, 260), (9, 8)]


@functools.lru_cache(maxsize=None)
def taps_case(taps, n):
    w = _lean(_rng('taps.w', taps, n), (taps, n))
    v = _lean(_rng('taps.v', taps, n), (n,))
    return SimpleNamespace(taps=taps, n=n, w=w, v=v, scale=TAPS_SCALE, sumsq=sumsq_taps(w), mul=bcast_mul_taps(w, v, TAPS_SCALE))


ROWS_SHAPES = [(count, M, L, D) for count in (1, 5, 24) for M, L, D in ((1, 3, 4), (3, 3, 128))]


def rows_case(count, M, L, D):
    """Slots 2, 0, 0, 2, 0, ...: repeats, and slot 1 named by nobody (its rows of `out` are exactly zero)."""
    src = _lean(_rng('rows.src', count, M, L, D), (count, M, D))
    slots = [2 if l % 3 == 0 else 0 for l in range(count)]
    assert 1 not in slots and L == 3
    return SimpleNamespace(count=count, M=M, L=L, D=D, src=src, slots=slots, ref=rows_group_sum(src, slots, L))


# ----------------------------------------------------------------------------- fp32 model of the forward kernel's summation
def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in fp64; one rounding to fp64 and one to fp32 (a model)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def prologue32(x, prologue, x2, ps):
    ps = np.float32(ps)
    if prologue == PRO_SQUARE:
        return x * x
    if prologue == PRO_DEMOD_GRAD:
        return ps * x * x2 * x2 * x2
    if prologue == PRO_MUL:
        return ps * x * x2
    return x


def dense_model32(c):
    """The kernel's arithmetic in fp32: 64 lane groups, group g takes the k-quads g, g + 64, ... with four fused multiply-adds per
    quad (innermost the quad's last element), the 64 partials are added in order, then alpha and the epilogue in fp32; the column
    sum adds the rows in order.  -> the same dict as dense()."""
    f = np.float32
    px = prologue32(c.x, c.prologue, c.x2, c.pro_scale).astype(f)
    M, K, N = c.M, c.K, c.N
    nq = K // 4
    acc = np.zeros((64, M, N), f)
    for q0 in range(0, nq, 64):
        g = np.arange(min(64, nq - q0))
        for e in (3, 2, 1, 0):
            k = (q0 + g) * 4 + e
            acc[g] = _fma32(px[:, k].T[:, :, None], c.W[k][:, None, :], acc[g])
    s = np.zeros((M, N), f)
    for g in range(64):
        s = s + acc[g]
    v = s * f(c.alpha)
    y2 = v
    if c.epilogue == EPI_SCALE:
        y = v
    elif c.epilogue == EPI_BIAS:
        y = v + (f(c.bias_scale) * c.bias[None, :] + f(c.add_const))
    elif c.epilogue == EPI_RSQRT:
        y = (f(1) / np.sqrt((v + f(c.eps)).astype(np.float64))).astype(f)
    elif c.epilogue == EPI_STYLE_GRAD:
        y = f(2) * c.e2 * v
        if c.e1 is not None:
            y = y + c.e1
    elif c.epilogue == EPI_DEMOD_GRAD2:
        d3 = c.e2 * c.e2 * c.e2
        y2 = f(0.75) * v * c.e1 * d3 * c.e2 * c.e2
        y = f(-0.5) * v * d3
    else:
        y = f(2) * _fma32(c.e2, v, c.e1 * c.e3)
    out = dict(y=y)
    if c.want_y2:
        out['y2'] = y2
    if c.want_colsum:
        t = np.zeros((N,), f)
        for m in range(M):
            t = t + y[m]
        out['colsum'] = f(c.bias_scale) * t
    return out


def wgrad_model32(c):
    """Rows in order, one fused multiply-add per row, alpha last."""
    f = np.float32
    a = prologue32(c.a, c.pro_a, None, 0.0).astype(f)
    b = prologue32(c.b, c.pro_b, c.b2, c.pro_scale).astype(f)
    acc = np.zeros((c.K, c.N), f)
    for m in range(c.M):
        acc = _fma32(a[m][:, None], b[m][None, :], acc)
    return acc * f(c.alpha)


def wgrad2_model32(c):
    """The two terms summed apart, rows in order, then alpha * first + alpha2 * second."""
    f = np.float32
    a = c.a if c.a2 is None else c.a * c.a2
    b = prologue32(c.b, c.pro_b, c.b2, c.pro_scale).astype(f)
    acc, acc2 = np.zeros((c.K, c.N), f), np.zeros((c.K, c.N), f)
    for m in range(c.M):
        acc = _fma32(a[m][:, None], b[m][None, :], acc)
        if c.c is not None:
            acc2 = _fma32(prologue32(c.c[m], c.pro_c, None, 0.0).astype(f)[:, None], c.d[m][None, :], acc2)
    return acc * f(c.alpha) + acc2 * f(c.alpha2)


# ----------------------------------------------------------------------------- guard-band arena
class Arena:
    """Every operand and output of a launch in ONE flat fp32 buffer at 16-byte-aligned offsets, 64-float guard bands of SENTINEL
    between them; outputs (and the padding columns of a strided y) start as SENTINEL too.  After the launch `violations` lists
    every guard float and every input float that changed; `out(flat, name)` is an output's region."""

    def __init__(self):
        self.spans = {}      # name -> (offset, shape, is_input)
        self.parts = []
        self.size = 0
        self._guard()

    def _guard(self):
        self.parts.append(np.full(GUARD, SENTINEL, np.float32))
        self.size += GUARD

    def _add(self, name, arr, is_input):
        assert name not in self.spans and self.size % 4 == 0
        self.spans[name] = (self.size, arr.shape, is_input)
        pad = (-arr.size) % 4
        self.parts.append(np.concatenate([arr.ravel(), np.full(pad, SENTINEL, np.float32)]))
        self.size += arr.size + pad
        self._guard()
        return self.spans[name][0]

    def put(self, name, arr):
        return self._add(name, np.asarray(arr, np.float32), True)

    def reserve(self, name, shape):
        return self._add(name, np.full(shape, SENTINEL, np.float32), False)

    def flat(self):
        return np.concatenate(self.parts)

    def offset(self, name):
        return self.spans[name][0]

    def addr(self, base, name, extra=0):
        """Device address of a tensor (+ `extra` floats) for a buffer at `base`; None for a tensor the case does not have."""
        return None if name not in self.spans else base + 4 * (self.spans[name][0] + extra)

    def out(self, flat, name):
        o, shape, _ = self.spans[name]
        return flat[o:o + int(np.prod(shape))].reshape(shape)

    def violations(self, before, after):
        bad = []
        mask = np.ones(self.size, bool)
        for name, (o, shape, is_input) in self.spans.items():
            n = int(np.prod(shape))
            mask[o:o + n] = False
            if is_input and not np.array_equal(before[o:o + n], after[o:o + n]):
                bad.append('input %s was written' % name)
        hit = np.flatnonzero(mask & (after != SENTINEL))
        if hit.size:
            names = sorted(self.spans, key=lambda k: self.spans[k][0])
            for i in hit[:4]:
                prev = [k for k in names if self.spans[k][0] <= i]
                bad.append('guard float %d (after %s) was written: %r' % (i, prev[-1] if prev else 'the start', float(after[i])))
        return bad


def place_dense(arena, c, tag=''):
    """A dense case's tensors into an arena (names prefixed with `tag`)."""
    arena.put(tag + 'x', c.x_full)
    arena.put(tag + 'w', c.w)
    for name in ('x2', 'bias', 'e1', 'e2', 'e3'):
        if getattr(c, name) is not None:
            arena.put(tag + name, getattr(c, name))
    arena.reserve(tag + 'y', (c.M, c.ldy))
    if c.want_y2:
        arena.reserve(tag + 'y2', (c.M, c.N))
    if c.want_colsum:
        arena.reserve(tag + 'colsum', (c.N,))


def dense_fields(arena, c, base, tag=''):
    """-> (fields of igan_dense_params, e3, y2) with device addresses for a buffer at `base`."""
    p = dict(x=arena.addr(base, tag + 'x', c.xoff), x2=arena.addr(base, tag + 'x2'), w=arena.addr(base, tag + 'w'), y=arena.addr(base, tag + 'y'),
             bias=arena.addr(base, tag + 'bias'), e1=arena.addr(base, tag + 'e1'), e2=arena.addr(base, tag + 'e2'),
             colsum=arena.addr(base, tag + 'colsum'), ldx=c.ldx, ldy=c.ldy, M=c.M, K=c.K, N=c.N, w_transposed=1 if c.wt else 0,
             prologue=c.prologue, epilogue=c.epilogue, alpha=c.alpha, pro_scale=c.pro_scale, bias_scale=c.bias_scale, add_const=c.add_const,
             eps=c.eps)
    return p, arena.addr(base, tag + 'e3'), arena.addr(base, tag + 'y2')


def dense_outputs(arena, c, flat, tag=''):
    """-> ({name: the kernel's output}, [complaints about the padding columns of y])."""
    yfull = arena.out(flat, tag + 'y')
    got = dict(y=yfull[:, :c.N])
    bad = [] if (yfull[:, c.N:] == SENTINEL).all() else ['padding columns N .. ldy - 1 of %sy were written' % tag]
    if c.want_y2:
        got['y2'] = arena.out(flat, tag + 'y2')
    if c.want_colsum:
        got['colsum'] = arena.out(flat, tag + 'colsum')
    return got, bad


def rel_err64(a, b):
    """tests.util.rel_err without torch: max|a - b| / (max|b| + 1e-30) in fp64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30)) if a.size else 0.0
