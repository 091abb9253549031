"""Host: (a) the inputs of tests/test_gpu_dense_small.py discriminate -- an fp32 model of the kernel's own summation
(dense_cases.dense_model32: 64 lane groups, four fused multiply-adds per k-quad, partials added in order) stays below a TENTH of every
bound of the GPU test on every case, and every mutant of the fp64 restatement listed below leaves the bound by a factor of 100 or
more on every case it applies to; (b) every entry point of csrc/dense_small.hip refuses bad arguments with a reason, before anything
reaches a device (NULL stream, dummy pointers: nothing here may launch)."""
import ctypes

import numpy as np
import pytest

import dense_cases as C

DENSE_FORMS = [(form, wt) for form in C.FORMS for wt in (False, True)]


def _worst(got, ref, bounds):
    """max over the outputs of rel_err / bound."""
    return max(C.rel_err64(got[k], ref[k]) / bounds[k] for k in ref)


# ----------------------------------------------------------------------------- (a) the model and the mutants
def _cut_rows(c, rows):
    cut = lambda t: None if t is None else t[:rows]
    return dict(x=c.x[:rows], x2=cut(c.x2), e1=cut(c.e1), e2=cut(c.e2), e3=cut(c.e3))


def _wrong_stride(c, t):
    """An [M, N] epilogue operand read at m * ldy + j (wrapped into the tensor: a model of the wrong index, not of what lies behind it)."""
    idx = (np.arange(c.M)[:, None] * c.ldy + np.arange(c.N)[None, :]) % t.size
    return t.ravel()[idx]


def dense_mutants(c):
    """{name: outputs of the mutated restatement} for the mutants that apply to this case."""
    K = c.K
    out = {}
    out['last k-quad dropped'] = C.dense_of(c, x=c.x[:, :K - 4], x2=None if c.x2 is None else c.x2[:, :K - 4],
                                            w=c.w[:, :K - 4] if c.wt else c.w[:K - 4])
    # row M - 1 neither staged nor written: the output row keeps the SENTINEL it was allocated with, the column sum lacks it
    m = C.dense_of(c, **_cut_rows(c, c.M - 1))
    sent = np.full((1, c.N), float(C.SENTINEL))
    out['row M-1 dropped'] = {k: (v if k == 'colsum' else np.concatenate([v, sent])) for k, v in m.items()}
    if c.ldy != c.N and c.M >= 2 and any(t is not None for t in (c.e1, c.e2, c.e3)):
        out['epilogue operands indexed with ldy'] = C.dense_of(c, **{k: _wrong_stride(c, getattr(c, k)) for k in ('e1', 'e2', 'e3') if getattr(c, k) is not None})
    if c.want_colsum:
        m = dict(c.ref)
        m['colsum'] = c.ref['colsum'] / c.bias_scale
        out['colsum without bias_scale'] = m
    if c.e1 is not None:
        out['e1 treated as absent'] = C.dense_of(c, e1=np.zeros_like(c.e1))
    if c.epilogue == C.EPI_DEMOD_GRAD2:
        out['y and y2 swapped'] = dict(y=c.ref['y2'], y2=c.ref['y'])
    return out


@pytest.mark.parametrize('form,wt', DENSE_FORMS)
def test_dense_inputs_discriminate(form, wt):
    bounds = C.bounds(form)
    worst_model, weakest, bad = 0.0, {}, []
    for shape in C.dense_shapes(form):
        c = C.dense_case(form, wt, *shape)
        r = _worst(C.dense_model32(c), c.ref, bounds)
        worst_model = max(worst_model, r)
        if not r < 0.1:
            bad.append(('model', shape, r))
        for name, m in dense_mutants(c).items():
            r = _worst(m, c.ref, bounds)
            weakest[name] = min(weakest.get(name, np.inf), r)
            if not r >= 100.0:
                bad.append((name, shape, r))
    print('%-18s wt %d: fp32 model at most %.3f of a bound; weakest mutants (x bound): %s'
          % (form, wt, worst_model, ', '.join('%s %.0f' % kv for kv in sorted(weakest.items()))))
    assert not bad, bad[:8]
    assert {'last k-quad dropped', 'row M-1 dropped'} <= set(weakest)
    assert ('epilogue operands indexed with ldy' in weakest) == (C.FORMS[form][1] >= C.EPI_STYLE_GRAD)


@pytest.mark.parametrize('table', ['GROUPED_BIAS', 'GROUPED_STYLE', 'GROUPED_SECOND'])
def test_grouped_inputs_discriminate(table):
    """The grouped launches' problems under the same model and mutants, and a launch that skips one group: that group's outputs keep
    the SENTINEL they were allocated with."""
    for wt in (False, True):
        for c in C.grouped_cases(getattr(C, table), wt):
            bounds = C.bounds(c.form)
            assert _worst(C.dense_model32(c), c.ref, bounds) < 0.1, (c.form, c.M, c.K, c.N)
            for name, m in dense_mutants(c).items():
                assert _worst(m, c.ref, bounds) >= 100.0, (name, c.form, c.M, c.K, c.N)
            skipped = {k: np.full(v.shape, float(C.SENTINEL)) for k, v in c.ref.items()}
            assert min(C.rel_err64(skipped[k], c.ref[k]) / bounds[k] for k in c.ref) >= 100.0, (c.form, c.M, c.K, c.N)


def test_wgrad_inputs_discriminate():
    bad, worst = [], 0.0
    for M, K, N, lda in C.wgrad_shapes():
        for pa, pb in C.wgrad_forms():
            c = C.wgrad_case(M, K, N, lda, pa, pb)
            r = C.rel_err64(C.wgrad_model32(c), c.ref) / C.BOUND_GRAD
            worst = max(worst, r)
            if not r < 0.1:
                bad.append(('model', M, K, N, pa, pb, r))
            muts = {'row M-1 dropped': M - 1}
            if M % 8:
                muts['rows at or above 8 floor(M / 8) dropped'] = 8 * (M // 8)
            for name, rows in muts.items():
                r = C.rel_err64(C.wgrad_of(c, rows), c.ref) / C.BOUND_GRAD
                if not r >= 100.0:
                    bad.append((name, M, K, N, pa, pb, r))
    print('wgrad: fp32 model at most %.3f of the bound' % worst)
    assert not bad, bad[:8]


def test_wgrad2_inputs_discriminate():
    bad, worst = [], 0.0
    for M, K, N, lda in C.wgrad_shapes():
        for a2, pb, pc in C.wgrad2_forms():
            for ldc in ((K, 3 * K) if pc is not None else (K,)):
                c = C.wgrad2_case(M, K, N, lda, ldc, a2, pb, pc)
                r = C.rel_err64(C.wgrad2_model32(c), c.ref) / C.BOUND_SECOND
                worst = max(worst, r)
                if not r < 0.1:
                    bad.append(('model', M, K, N, a2, pb, pc, r))
                muts = {'row M-1 dropped': M - 1}
                if M % 8:
                    muts['rows at or above 8 floor(M / 8) dropped'] = 8 * (M // 8)
                for name, rows in muts.items():
                    r = C.rel_err64(C.wgrad2_of(c, rows), c.ref) / C.BOUND_SECOND
                    if not r >= 100.0:
                        bad.append((name, M, K, N, a2, pb, pc, r))
                if pc is not None:      # alpha2 differs from alpha: a kernel that scales both terms by alpha shows
                    same = C.wgrad2(c.a, c.a2, c.b, c.b2, c.c, c.d, alpha=c.alpha, alpha2=c.alpha, pro_b=c.pro_b, pro_c=c.pro_c, pro_scale=c.pro_scale)
                    r = C.rel_err64(same, c.ref) / C.BOUND_SECOND
                    if not r >= 100.0:
                        bad.append(('alpha2 = alpha', M, K, N, a2, pb, pc, r))
    print('wgrad2: fp32 model at most %.3f of the bound' % worst)
    assert not bad, bad[:8]


def test_taps_inputs_are_plain():
    """One fp32 product (and at most nine fused additions) per element: the model is far inside the bound; a tap or a lane left
    out is not."""
    for taps, n in C.TAPS_SHAPES + C.TAPS_GROUPED:
        c = C.taps_case(taps, n)
        s = np.zeros((n,), np.float32)
        for t in range(taps):
            s = C._fma32(c.w[t], c.w[t], s)
        assert C.rel_err64(s, c.sumsq) < 0.1 * C.BOUND_GRAD and C.rel_err64(np.float32(c.scale) * c.w * c.v[None, :], c.mul) < 0.1 * C.BOUND_GRAD
        assert C.rel_err64(C.sumsq_taps(c.w[:taps - 1]), c.sumsq) >= 100 * C.BOUND_GRAD
        lost = c.sumsq.copy()
        lost[-4:] = float(C.SENTINEL)      # the last lane's four outputs never written
        assert C.rel_err64(lost, c.sumsq) >= 100 * C.BOUND_GRAD


def test_rows_group_sum_reference_is_an_in_order_fp32_sum():
    for shape in C.ROWS_SHAPES:
        c = C.rows_case(*shape)
        assert c.ref.dtype == np.float32 and not c.ref[:, 1].any()
        want = np.zeros_like(c.ref)
        for m in range(c.M):
            for j in (0, 2):
                rows = [c.src[l, m] for l in range(c.count) if c.slots[l] == j]
                if rows:
                    want[m, j] = np.cumsum(np.stack(rows), axis=0, dtype=np.float32)[-1]
        assert np.array_equal(c.ref, want)
    assert {len(set(C.rows_case(*s).slots)) for s in C.ROWS_SHAPES} == {1, 2}


def test_arena_keeps_alignment_and_finds_a_stray_write():
    a = C.Arena()
    a.put('x', np.ones((3, 5), np.float32))
    a.reserve('y', (2, 7))
    flat = a.flat()
    assert flat.size == a.size and all(o % 4 == 0 for o, _, _ in a.spans.values())
    assert a.offset('y') - (a.offset('x') + 16) == C.GUARD and (a.out(flat, 'y') == C.SENTINEL).all()
    after = flat.copy()
    a.out(after, 'y')[:] = 1.0
    assert a.violations(flat, after) == []
    after[a.offset('y') + 14] = 0.0            # the float behind y's 14: alignment padding, part of the guard
    after[a.offset('x')] = 2.0
    assert len(a.violations(flat, after)) == 2


# ----------------------------------------------------------------------------- (b) argument checks
A = 1 << 20      # a 16-byte-aligned address that is never dereferenced: validation fails first
OFF = A + 4      # 4-byte aligned only


def _lib():
    from inclusivegan_amd import _abi
    return _abi, _abi.get_plugin()


def _refused(rc, needle):
    _abi, lib = _lib()
    msg = lib.igan_last_error()
    assert rc == _abi.IGAN_ERR_INVALID_ARGUMENT and needle.encode() in msg, (rc, needle, msg)


def _dense_params(**over):
    _abi, _ = _lib()
    kw = dict(x=A, x2=None, w=A, y=A, bias=None, e1=None, e2=None, colsum=None, ldx=8, ldy=4, M=2, K=8, N=4, w_transposed=0,
              prologue=C.PRO_NONE, epilogue=C.EPI_SCALE, alpha=1.0, pro_scale=1.0, bias_scale=1.0, add_const=0.0, eps=0.0)
    kw.update(over)
    return _abi.DenseParams(**kw)


# what both dense entry-point families refuse: (fields, reason)
DENSE_BAD = [
    (dict(M=0), '1 <= M <= 64'), (dict(M=65), '1 <= M <= 64'),
    (dict(K=0, ldx=0), 'K must be a positive multiple of 4'), (dict(K=6, ldx=8), 'K must be a positive multiple of 4'),
    (dict(N=0, ldy=0), 'N positive'),
    (dict(ldx=4), 'bad row strides'), (dict(ldx=10), 'bad row strides'), (dict(ldy=3), 'bad row strides'),
    (dict(x=OFF), '16-byte aligned'), (dict(w=OFF, w_transposed=1), '16-byte aligned'),
    (dict(prologue=C.PRO_DEMOD_GRAD, x2=OFF), 'aligned x2'), (dict(prologue=C.PRO_DEMOD_GRAD), 'aligned x2'),
    (dict(prologue=-1), 'unknown prologue'), (dict(epilogue=-1), 'unknown epilogue'),
    (dict(epilogue=C.EPI_BIAS), 'needs a bias'),
    (dict(epilogue=C.EPI_STYLE_GRAD, e1=A), 'needs e2'),
    (dict(x=None), 'null buffer'), (dict(w=None), 'null buffer'), (dict(y=None), 'null buffer'),
]
# the first-order entry points know neither MUL nor the second-order epilogues
DENSE1_BAD = [
    (dict(prologue=C.PRO_MUL, x2=A), 'unknown prologue'),
    (dict(epilogue=C.EPI_DEMOD_GRAD2, e1=A, e2=A), 'unknown epilogue'),
    (dict(epilogue=C.EPI_STYLE_GRAD2, e1=A, e2=A), 'unknown epilogue'),
]
# igan_dense_small2_grouped: (fields, e3, y2, reason)
DENSE2_BAD = [
    (dict(prologue=4), None, None, 'unknown prologue'), (dict(epilogue=6), None, None, 'unknown epilogue'),
    (dict(prologue=C.PRO_MUL), None, None, 'aligned x2'), (dict(prologue=C.PRO_MUL, x2=OFF), None, None, 'aligned x2'),
    (dict(epilogue=C.EPI_DEMOD_GRAD2, e2=A), None, A, 'needs e1, e2 and y2'),
    (dict(epilogue=C.EPI_DEMOD_GRAD2, e1=A), None, A, 'needs e1, e2 and y2'),
    (dict(epilogue=C.EPI_DEMOD_GRAD2, e1=A, e2=A), None, None, 'needs e1, e2 and y2'),
    (dict(epilogue=C.EPI_STYLE_GRAD2, e1=A, e2=A), None, A, 'needs e1, e2 and e3'),
    (dict(epilogue=C.EPI_STYLE_GRAD2, e2=A), A, None, 'needs e1, e2 and e3'),
    (dict(epilogue=C.EPI_STYLE_GRAD2, e1=A), A, None, 'needs e1, e2 and e3'),
]


def test_dense_entry_points_refuse_bad_arguments():
    _abi, lib = _lib()
    for over, why in DENSE_BAD + DENSE1_BAD:
        p = _dense_params(**over)
        _refused(lib.igan_dense_small(None, ctypes.byref(p)), why)
        _refused(lib.igan_dense_small_grouped(None, (_abi.DenseParams * 1)(p), 1), why)
        _refused(lib.igan_dense_small_grouped(None, (_abi.DenseParams * 2)(_dense_params(), p), 2), why)      # every group is checked before the launch
    for over, e3, y2, why in [(o, None, None, w) for o, w in DENSE_BAD] + DENSE2_BAD:
        g = _abi.Dense2Params(p=_dense_params(**over), e3=e3, y2=y2)
        _refused(lib.igan_dense_small2_grouped(None, (_abi.Dense2Params * 1)(g), 1), why)
        good = _abi.Dense2Params(p=_dense_params(), e3=None, y2=None)
        _refused(lib.igan_dense_small2_grouped(None, (_abi.Dense2Params * 2)(good, g), 2), why)
    # the group count, a missing list, and groups of two weight layouts
    some = (_abi.DenseParams * 25)(*[_dense_params() for _ in range(25)])
    some2 = (_abi.Dense2Params * 25)(*[_abi.Dense2Params(p=_dense_params(), e3=None, y2=None) for _ in range(25)])
    for count in (0, 25, -1):
        _refused(lib.igan_dense_small_grouped(None, some, count), 'count <= 24')
        _refused(lib.igan_dense_small2_grouped(None, some2, count), 'count <= 24')
    _refused(lib.igan_dense_small_grouped(None, None, 1), 'count <= 24')
    _refused(lib.igan_dense_small2_grouped(None, None, 1), 'count <= 24')
    mixed = (_abi.DenseParams * 2)(_dense_params(), _dense_params(w_transposed=1))
    _refused(lib.igan_dense_small_grouped(None, mixed, 2), 'share w_transposed')
    mixed2 = (_abi.Dense2Params * 2)(_abi.Dense2Params(p=_dense_params(w_transposed=1)), _abi.Dense2Params(p=_dense_params()))
    _refused(lib.igan_dense_small2_grouped(None, mixed2, 2), 'share w_transposed')


def _wgrad_params(**over):
    _abi, _ = _lib()
    kw = dict(a=A, b=A, b2=None, dw=A, lda=8, M=2, K=8, N=4, pro_a=C.PRO_NONE, pro_b=C.PRO_NONE, alpha=1.0, pro_scale=1.0)
    kw.update(over)
    return _abi.DenseWgradParams(**kw)


def _wgrad2_params(**over):
    _abi, _ = _lib()
    kw = dict(a=A, a2=None, b=A, b2=None, c=None, d=None, dw=A, lda=8, ldc=8, M=2, K=8, N=4, pro_b=C.PRO_NONE, pro_c=C.PRO_NONE, alpha=1.0,
              pro_scale=1.0, alpha2=1.0)
    kw.update(over)
    return _abi.DenseWgrad2Params(**kw)


WGRAD_BAD = [      # both weight-gradient families
    (dict(M=0), '1 <= M <= 64'), (dict(M=65), '1 <= M <= 64'),
    (dict(N=6), 'N must be a positive multiple of 4'), (dict(N=0), 'N must be a positive multiple of 4'),
    (dict(K=0), 'N must be a positive multiple of 4'), (dict(lda=4), 'N must be a positive multiple of 4'),
    (dict(b=OFF), '16-byte aligned'), (dict(dw=OFF), '16-byte aligned'),
    (dict(pro_b=C.PRO_DEMOD_GRAD, b2=OFF), 'bad prologue for b'), (dict(pro_b=C.PRO_DEMOD_GRAD), 'bad prologue for b'),
    (dict(pro_b=C.PRO_SQUARE), 'bad prologue for b'),
    (dict(a=None), 'null buffer'), (dict(b=None), 'null buffer'), (dict(dw=None), 'null buffer'),
]


def test_wgrad_entry_points_refuse_bad_arguments():
    _abi, lib = _lib()
    for over, why in WGRAD_BAD + [(dict(pro_a=C.PRO_DEMOD_GRAD), 'unknown prologue for a')]:
        p = _wgrad_params(**over)
        _refused(lib.igan_dense_small_wgrad(None, ctypes.byref(p)), why)
        _refused(lib.igan_dense_small_wgrad_grouped(None, (_abi.DenseWgradParams * 2)(_wgrad_params(), p), 2), why)
    for over, why in WGRAD_BAD + [(dict(c=A), 'null buffer'), (dict(c=A, d=A, ldc=4), 'N must be a positive multiple of 4'),
                                  (dict(c=A, d=OFF), '16-byte aligned'), (dict(pro_c=C.PRO_DEMOD_GRAD), 'unknown prologue for c')]:
        p = _wgrad2_params(**over)
        _refused(lib.igan_dense_small_wgrad2_grouped(None, (_abi.DenseWgrad2Params * 2)(_wgrad2_params(), p), 2), why)
    some = (_abi.DenseWgradParams * 25)(*[_wgrad_params() for _ in range(25)])
    some2 = (_abi.DenseWgrad2Params * 25)(*[_wgrad2_params() for _ in range(25)])
    for count in (0, 25):
        _refused(lib.igan_dense_small_wgrad_grouped(None, some, count), 'count <= 24')
        _refused(lib.igan_dense_small_wgrad2_grouped(None, some2, count), 'count <= 24')
    _refused(lib.igan_dense_small_wgrad_grouped(None, None, 1), 'count <= 24')
    _refused(lib.igan_dense_small_wgrad2_grouped(None, None, 1), 'count <= 24')


def test_taps_and_rows_entry_points_refuse_bad_arguments():
    _abi, lib = _lib()
    T = _abi.TapsParams
    for w, v, out, taps, n, why in [(A, A, A, 3, 6, 'n must be a positive multiple of 4'), (A, A, A, 3, 0, 'n must be a positive multiple of 4'),
                                    (A, A, A, 0, 4, 'n must be a positive multiple of 4'), (None, A, A, 3, 4, 'n must be a positive multiple of 4'),
                                    (A, A, None, 3, 4, 'n must be a positive multiple of 4'),
                                    (OFF, A, A, 3, 4, 'buffers must be 16-byte aligned'), (A, A, OFF, 3, 4, 'buffers must be 16-byte aligned')]:
        _refused(lib.igan_sumsq_taps(None, w, out, taps, n), 'sumsq_taps: ' + why)
        _refused(lib.igan_bcast_mul_taps(None, w, v, out, taps, n, 2.0), 'bcast_mul_taps: ' + why)
        good, g = T(w=A, v=A, out=A, taps=3, n=4, scale=2.0), T(w=w, v=v, out=out, taps=taps, n=n, scale=2.0)
        _refused(lib.igan_sumsq_taps_grouped(None, (T * 2)(good, g), 2), 'sumsq_taps: ' + why)
        _refused(lib.igan_bcast_mul_taps_grouped(None, (T * 2)(good, g), 2), 'bcast_mul_taps: ' + why)
    _refused(lib.igan_bcast_mul_taps(None, A, None, A, 3, 4, 2.0), 'bcast_mul_taps: n must be')      # the factor is missing
    _refused(lib.igan_bcast_mul_taps(None, A, OFF, A, 3, 4, 2.0), 'bcast_mul_taps: buffers must be 16-byte aligned')
    some = (T * 25)(*[T(w=A, v=A, out=A, taps=3, n=4, scale=2.0) for _ in range(25)])
    for count in (0, 25):
        _refused(lib.igan_sumsq_taps_grouped(None, some, count), 'count <= 24')
        _refused(lib.igan_bcast_mul_taps_grouped(None, some, count), 'count <= 24')
    # igan_rows_group_sum: the count, D, alignment, and a slot outside [0, L)
    slots = (ctypes.c_int * 25)(*([0, 2] * 12 + [0]))
    for count in (0, 25):
        _refused(lib.igan_rows_group_sum(None, A, slots, count, A, 2, 3, 8), 'count <= 24')
    _refused(lib.igan_rows_group_sum(None, A, None, 2, A, 2, 3, 8), 'count <= 24')
    for M, L, D in ((0, 3, 8), (2, 0, 8), (2, 3, 6), (2, 3, 0)):
        _refused(lib.igan_rows_group_sum(None, A, slots, 2, A, M, L, D), 'D must be a positive multiple of 4')
    _refused(lib.igan_rows_group_sum(None, OFF, slots, 2, A, 2, 3, 8), '16-byte aligned')
    _refused(lib.igan_rows_group_sum(None, A, slots, 2, OFF, 2, 3, 8), '16-byte aligned')
    for bad in (3, -1, 1 << 20):
        s = (ctypes.c_int * 3)(0, bad, 2)
        _refused(lib.igan_rows_group_sum(None, A, s, 3, A, 2, 3, 8), 'slot[1] = %d is outside [0, 3)' % bad)
    _refused(lib.igan_rows_group_sum(None, A, (ctypes.c_int * 2)(0, 2), 2, A, 2, 2, 8), 'slot[1] = 2 is outside [0, 2)')
