"""GPU: every form of the small dense kernels (csrc/dense_small.hip) at the C ABI against the fp64 restatement of
tests/dense_cases.py, at the smallest shapes that reach each branch: all six row buckets and their edges, one k-quad, one quad past
the 256- and the 512-float reduction super-tile, a quarter-filled and a one-column last workgroup, a strided x (the [:, 1] slice of
[M, 3, K]) and a padded y, both weight layouts, up to 24 problems of different sizes in one launch.

The structs are built here, so ldy, y2, e3 and the group lists are the test's.  Every operand and output of a launch lies in ONE flat
device buffer between 64-float guard bands of a finite sentinel (dense_cases.Arena); outputs and the padding columns of y start as the
sentinel.  After each launch every guard float and every input must be unchanged: an out-of-range write at a ragged N shows without
anything being provoked.  A test loops over its shapes and collects every failure before it asserts; it prints its largest error per
output.  Bounds: dense_cases.BOUND_* (the issue's table: the limits the callers' own tests hold these quantities to).  Grouped
launches are compared per group with fp64, bit for bit with the same problem launched in the same row bucket on its own, and run twice
("Deterministic" in the header); igan_rows_group_sum bit for bit with an in-order fp32 sum."""
import ctypes

import numpy as np
import pytest
import torch

import dense_cases as C

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


class Launch:
    """An arena on the device: upload, launch through `call(base address)`, read back, list guard violations."""

    def __init__(self, arena, dev):
        self.arena = arena
        self.before = arena.flat()
        self.buf = torch.from_numpy(self.before).to(dev)
        assert self.buf.data_ptr() % 16 == 0
        self.base = self.buf.data_ptr()
        self.after = None

    def run(self, call):
        from inclusivegan_amd import _abi
        _abi.check(call())
        torch.cuda.synchronize()
        self.after = self.buf.cpu().numpy()
        return self.arena.violations(self.before, self.after)


def _stream():
    from inclusivegan_amd import hip_ops
    return hip_ops._stream()


def dense_launch(dev, cases):
    """One launch of `cases` (tags g0., g1., ...): igan_dense_small for one first-order problem, igan_dense_small_grouped for several,
    igan_dense_small2_grouped as soon as one problem is a second-order form.  -> (Launch, complaints)."""
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    arena = C.Arena()
    for i, c in enumerate(cases):
        C.place_dense(arena, c, 'g%d.' % i)
    L = Launch(arena, dev)
    fields = [C.dense_fields(arena, c, L.base, 'g%d.' % i) for i, c in enumerate(cases)]
    if any(c.entry == 2 for c in cases):
        arr = (_abi.Dense2Params * len(cases))(*[_abi.Dense2Params(p=_abi.DenseParams(**p), e3=e3, y2=y2) for p, e3, y2 in fields])
        bad = L.run(lambda: lib.igan_dense_small2_grouped(_stream(), arr, len(cases)))
    elif len(cases) == 1:
        p = _abi.DenseParams(**fields[0][0])
        bad = L.run(lambda: lib.igan_dense_small(_stream(), ctypes.byref(p)))
    else:
        arr = (_abi.DenseParams * len(cases))(*[_abi.DenseParams(**p) for p, _, _ in fields])
        bad = L.run(lambda: lib.igan_dense_small_grouped(_stream(), arr, len(cases)))
    return L, bad


def dense_check(L, cases, fails, worst, where):
    """Every group's outputs against fp64; -> [{name: output}] per group."""
    outs = []
    for i, c in enumerate(cases):
        got, bad = C.dense_outputs(L.arena, c, L.after, 'g%d.' % i)
        fails += [(where, i, b) for b in bad]
        bounds = C.bounds(c.form)
        for k, ref in c.ref.items():
            if not np.isfinite(got[k]).all():
                fails.append((where, i, k, 'not finite'))
                continue
            e = C.rel_err64(got[k], ref)
            key = (c.form, k)
            worst[key] = max(worst.get(key, 0.0), e)
            if not e < bounds[k]:
                fails.append((where, i, c.form, k, e, bounds[k]))
        outs.append(got)
    return outs


def _report(title, worst, bound_of):
    for key in sorted(worst):
        print('%-34s %-26s largest rel_err %.3e  bound %.0e%s' % (title, '%s %s' % key if isinstance(key, tuple) else key, worst[key], bound_of(key),
                                                                    '' if worst[key] <= 0.5 * bound_of(key) else
                                                                    '  (within 2x of the bound)' if worst[key] < bound_of(key) else '  (ABOVE the bound)'))


def bucket(M, wt):
    """The row bucket a launch whose largest problem has M rows runs in, from the library (the plain 1x1-convolution form reports its
    kernel; the bucket is a function of M alone: dense_small_rows)."""
    from inclusivegan_amd import _abi
    p = _abi.Conv2DParams(x=1 << 20, w=1 << 20, y=1 << 20, in_scale=None, out_scale=None, workspace=None, workspace_floats=0, N=M, H=1, W=1, Cin=8,
                          OH=1, OW=1, Cout=4, KH=1, KW=1, stride=1, up=1, pad_y=0, pad_x=0, w_transposed=1 if wt else 0, splits=1, alpha=1.0, bias=None,
                          act=0, act_alpha=0.0, act_gain=1.0)
    buf = ctypes.create_string_buffer(128)
    _abi.check(_abi.get_plugin().igan_conv2d_kernel_name(ctypes.byref(p), buf, 128))
    name = buf.value.decode()
    assert name.startswith('dense_small_kernel<') and name.endswith(', %s>' % ('true' if wt else 'false')), name
    return int(name[len('dense_small_kernel<'):].split(',')[0])


# ----------------------------------------------------------------------------- forward kernel, single launches
@pytest.mark.parametrize('wt', [False, True], ids=['w_kn', 'w_nk'])
@pytest.mark.parametrize('form', list(C.FORMS))
def test_dense_single_launch(cuda_device, form, wt):
    fails, worst = [], {}
    for shape in C.dense_shapes(form):
        c = C.dense_case(form, wt, *shape)
        L, bad = dense_launch(cuda_device, [c])
        fails += [(shape, b) for b in bad]
        dense_check(L, [c], fails, worst, shape)
    _report('dense %s' % ('w[n][k]' if wt else 'w[k][n]'), worst, lambda key: C.bounds(key[0])[key[1]])
    assert not fails, (len(fails), fails[:6])


def test_buckets_are_the_six_of_the_kernel():
    assert [bucket(M, False) for M in (1, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 64)] == [8, 8, 16, 16, 24, 24, 32, 32, 48, 48, 64, 64]
    assert bucket(33, True) == 48


# ----------------------------------------------------------------------------- grouped launches
@pytest.mark.parametrize('table,wt', [('GROUPED_BIAS', False), ('GROUPED_BIAS', True), ('GROUPED_STYLE', True), ('GROUPED_SECOND', False),
                                      ('GROUPED_SECOND', True)])
def test_dense_grouped_launch(cuda_device, table, wt):
    cases = C.grouped_cases(getattr(C, table), wt)
    assert len({(c.M, c.K, c.N) for c in cases}) == len(cases)
    fails, worst = [], {}
    L, bad = dense_launch(cuda_device, cases)
    fails += [('grouped', b) for b in bad]
    outs = dense_check(L, cases, fails, worst, 'grouped')
    # twice into fresh outputs: the whole buffers are equal, bits included
    L2, bad = dense_launch(cuda_device, cases)
    fails += [('second run', b) for b in bad]
    if not torch.equal(L.buf.view(torch.int32), L2.buf.view(torch.int32)):
        fails.append(('two runs differ',))
    # each group bit for bit against the same problem in a launch of the same row bucket: on its own where its own M reaches that
    # bucket, else beside a one-column filler of the launch's largest M (group 0 of that launch is the problem)
    maxM = max(c.M for c in cases)
    mb = bucket(maxM, wt)
    filler = C.dense_case('scale', wt, maxM, 4, 1)
    for i, c in enumerate(cases):
        solo = [c] if bucket(c.M, wt) == mb else [c, filler]
        Ls, bad = dense_launch(cuda_device, solo)
        fails += [('solo', i, b) for b in bad]
        got, _ = C.dense_outputs(Ls.arena, c, Ls.after, 'g0.')
        for k in got:
            if not _bits_equal(got[k], outs[i][k]):
                fails.append(('group %d (%s M %d K %d N %d) %s differs from its solo launch' % (i, c.form, c.M, c.K, c.N, k),
                              C.rel_err64(got[k], outs[i][k])))
    _report('%s %s, %d groups' % (table, 'w[n][k]' if wt else 'w[k][n]', len(cases)), worst, lambda key: C.bounds(key[0])[key[1]])
    assert not fails, (len(fails), fails[:6])


# ----------------------------------------------------------------------------- weight gradients
def _place_wgrad(arena, c, tag, second):
    arena.put(tag + 'a', c.a_full)
    arena.put(tag + 'b', c.b)
    for name in ('b2',) + (('a2', 'd') if second else ()):
        if getattr(c, name) is not None:
            arena.put(tag + name, getattr(c, name))
    if second and c.c_full is not None:
        arena.put(tag + 'c', c.c_full)
    arena.reserve(tag + 'dw', (c.K, c.N))


def _wgrad_struct(arena, c, base, tag, second):
    from inclusivegan_amd import _abi
    if not second:
        return _abi.DenseWgradParams(a=arena.addr(base, tag + 'a', c.aoff), b=arena.addr(base, tag + 'b'), b2=arena.addr(base, tag + 'b2'),
                                     dw=arena.addr(base, tag + 'dw'), lda=c.lda, M=c.M, K=c.K, N=c.N, pro_a=c.pro_a, pro_b=c.pro_b, alpha=c.alpha,
                                     pro_scale=c.pro_scale)
    return _abi.DenseWgrad2Params(a=arena.addr(base, tag + 'a', c.aoff), a2=arena.addr(base, tag + 'a2'), b=arena.addr(base, tag + 'b'),
                                  b2=arena.addr(base, tag + 'b2'), c=arena.addr(base, tag + 'c', c.coff), d=arena.addr(base, tag + 'd'),
                                  dw=arena.addr(base, tag + 'dw'), lda=c.lda, ldc=c.ldc, M=c.M, K=c.K, N=c.N, pro_b=c.pro_b, pro_c=c.pro_c,
                                  alpha=c.alpha, pro_scale=c.pro_scale, alpha2=c.alpha2)


def wgrad_launch(dev, cases, second, single=False):
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    arena = C.Arena()
    for i, c in enumerate(cases):
        _place_wgrad(arena, c, 'g%d.' % i, second)
    L = Launch(arena, dev)
    structs = [_wgrad_struct(arena, c, L.base, 'g%d.' % i, second) for i, c in enumerate(cases)]
    if single:
        bad = L.run(lambda: lib.igan_dense_small_wgrad(_stream(), ctypes.byref(structs[0])))
    else:
        arr = ((_abi.DenseWgrad2Params if second else _abi.DenseWgradParams) * len(cases))(*structs)
        fn = lib.igan_dense_small_wgrad2_grouped if second else lib.igan_dense_small_wgrad_grouped
        bad = L.run(lambda: fn(_stream(), arr, len(cases)))
    return L, bad


def _wgrad_check(L, cases, bound, fails, where):
    worst = 0.0
    for i, c in enumerate(cases):
        got = L.arena.out(L.after, 'g%d.dw' % i)
        e = C.rel_err64(got, c.ref) if np.isfinite(got).all() else np.inf
        worst = max(worst, e)
        if not e < bound:
            fails.append((where, i, (c.M, c.K, c.N), e, bound))
    return worst


@pytest.mark.parametrize('pro_a,pro_b', C.wgrad_forms())
def test_wgrad_single_launch(cuda_device, pro_a, pro_b):
    fails, worst = [], 0.0
    for M, K, N, lda in C.wgrad_shapes():
        c = C.wgrad_case(M, K, N, lda, pro_a, pro_b)
        L, bad = wgrad_launch(cuda_device, [c], False, single=True)
        fails += [((M, K, N, lda), b) for b in bad]
        worst = max(worst, _wgrad_check(L, [c], C.BOUND_GRAD, fails, (M, K, N, lda)))
    _report('wgrad', {'pro_a %d pro_b %d' % (pro_a, pro_b): worst}, lambda key: C.BOUND_GRAD)
    assert not fails, (len(fails), fails[:6])


@pytest.mark.parametrize('has_a2,pro_b,pro_c', C.wgrad2_forms())
def test_wgrad2_single_group(cuda_device, has_a2, pro_b, pro_c):
    fails, worst = [], 0.0
    for M, K, N, lda in C.wgrad_shapes():
        for ldc in ((K, 3 * K) if pro_c is not None else (K,)):
            c = C.wgrad2_case(M, K, N, lda, ldc, has_a2, pro_b, pro_c)
            L, bad = wgrad_launch(cuda_device, [c], True)
            fails += [((M, K, N, lda, ldc), b) for b in bad]
            worst = max(worst, _wgrad_check(L, [c], C.BOUND_SECOND, fails, (M, K, N, lda, ldc)))
    _report('wgrad2', {'a2 %d pro_b %d pro_c %s' % (has_a2, pro_b, pro_c): worst}, lambda key: C.BOUND_SECOND)
    assert not fails, (len(fails), fails[:6])


@pytest.mark.parametrize('second', [False, True], ids=['wgrad', 'wgrad2'])
def test_wgrad_grouped_launch(cuda_device, second):
    """Six groups of different K * N in one launch: the thread-index guard ends some lanes early in some groups only."""
    if second:
        forms = C.wgrad2_forms()
        cases = [C.wgrad2_case(M, K, N, 3 * K if i % 2 else K, K if i % 3 else 3 * K, *forms[(5 * i + 2) % len(forms)]) for i, (M, K, N) in enumerate(C.WGRAD_GROUPED)]
    else:
        forms = C.wgrad_forms()
        cases = [C.wgrad_case(M, K, N, 3 * K if i % 2 else K, *forms[i % len(forms)]) for i, (M, K, N) in enumerate(C.WGRAD_GROUPED)]
    assert len({c.K * c.N for c in cases}) == len(cases)
    bound = C.BOUND_SECOND if second else C.BOUND_GRAD
    fails = []
    L, bad = wgrad_launch(cuda_device, cases, second)
    fails += [('grouped', b) for b in bad]
    worst = _wgrad_check(L, cases, bound, fails, 'grouped')
    L2, bad = wgrad_launch(cuda_device, cases, second)
    fails += [('second run', b) for b in bad]
    if not torch.equal(L.buf.view(torch.int32), L2.buf.view(torch.int32)):
        fails.append(('two runs differ',))
    for i, c in enumerate(cases):      # the same problem alone: the same rows in the same order
        Ls, bad = wgrad_launch(cuda_device, [c], second)
        fails += [('solo', i, b) for b in bad]
        if not _bits_equal(Ls.arena.out(Ls.after, 'g0.dw'), L.arena.out(L.after, 'g%d.dw' % i)):
            fails.append(('group %d differs from its solo launch' % i,))
    _report('wgrad2 grouped' if second else 'wgrad grouped', {'6 groups': worst}, lambda key: bound)
    assert not fails, (len(fails), fails[:6])


# ----------------------------------------------------------------------------- taps
def taps_launch(dev, cases, mul, single):
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    arena = C.Arena()
    for i, c in enumerate(cases):
        arena.put('g%d.w' % i, c.w)
        if mul:
            arena.put('g%d.v' % i, c.v)
        arena.reserve('g%d.out' % i, (c.taps, c.n) if mul else (c.n,))
    L = Launch(arena, dev)
    ad = lambda i, name: arena.addr(L.base, 'g%d.%s' % (i, name))
    if single:
        c = cases[0]
        if mul:
            bad = L.run(lambda: lib.igan_bcast_mul_taps(_stream(), ad(0, 'w'), ad(0, 'v'), ad(0, 'out'), c.taps, c.n, c.scale))
        else:
            bad = L.run(lambda: lib.igan_sumsq_taps(_stream(), ad(0, 'w'), ad(0, 'out'), c.taps, c.n))
    else:
        arr = (_abi.TapsParams * len(cases))(*[_abi.TapsParams(w=ad(i, 'w'), v=ad(i, 'v'), out=ad(i, 'out'), taps=c.taps, n=c.n, scale=c.scale)
                                               for i, c in enumerate(cases)])
        fn = lib.igan_bcast_mul_taps_grouped if mul else lib.igan_sumsq_taps_grouped
        bad = L.run(lambda: fn(_stream(), arr, len(cases)))
    return L, bad


@pytest.mark.parametrize('mul', [False, True], ids=['sumsq_taps', 'bcast_mul_taps'])
def test_taps(cuda_device, mul):
    fails, worst = [], {}

    def check(L, cases, where):
        for i, c in enumerate(cases):
            got = L.arena.out(L.after, 'g%d.out' % i)
            e = C.rel_err64(got, c.mul if mul else c.sumsq) if np.isfinite(got).all() else np.inf
            worst[where] = max(worst.get(where, 0.0), e)
            if not e < C.BOUND_GRAD:
                fails.append((where, i, (c.taps, c.n), e))

    for taps, n in C.TAPS_SHAPES:
        L, bad = taps_launch(cuda_device, [C.taps_case(taps, n)], mul, True)
        fails += [((taps, n), b) for b in bad]
        check(L, [C.taps_case(taps, n)], 'single')
    cases = [C.taps_case(t, n) for t, n in C.TAPS_GROUPED]
    L, bad = taps_launch(cuda_device, cases, mul, False)
    fails += [('grouped', b) for b in bad]
    check(L, cases, 'grouped')
    L2, bad = taps_launch(cuda_device, cases, mul, False)
    fails += [('second run', b) for b in bad]
    if not torch.equal(L.buf.view(torch.int32), L2.buf.view(torch.int32)):
        fails.append(('two runs differ',))
    _report('bcast_mul_taps' if mul else 'sumsq_taps', worst, lambda key: C.BOUND_GRAD)
    assert not fails, (len(fails), fails[:6])


# ----------------------------------------------------------------------------- igan_rows_group_sum
def test_rows_group_sum_is_an_in_order_sum(cuda_device):
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    fails = []
    for shape in C.ROWS_SHAPES:
        c = C.rows_case(*shape)
        arena = C.Arena()
        arena.put('src', c.src)
        arena.reserve('out', (c.M, c.L, c.D))
        slots = (ctypes.c_int * c.count)(*c.slots)
        runs = []
        for _ in range(2):
            L = Launch(arena, cuda_device)
            fails += [(shape, b) for b in L.run(lambda: lib.igan_rows_group_sum(_stream(), arena.addr(L.base, 'src'), slots, c.count,
                                                                                arena.addr(L.base, 'out'), c.M, c.L, c.D))]
            runs.append(L.arena.out(L.after, 'out'))
        if not _bits_equal(runs[0], c.ref):
            fails.append((shape, 'differs from the in-order fp32 sum', C.rel_err64(runs[0], c.ref)))
        if not _bits_equal(runs[0][:, 1], np.zeros((c.M, c.D), np.float32)):
            fails.append((shape, 'the slot nobody names is not exactly zero'))
        if not _bits_equal(runs[0], runs[1]):
            fails.append((shape, 'two runs differ'))
    assert not fails, (len(fails), fails[:6])


# ----------------------------------------------------------------------------- StyleModAllFn, first order
STYLE_LAYERS = [(36, 20, 3, True), (12, 8, 1, True), (36, 3, 1, False), (260, 12, 3, True)]      # Cin, Cout, filter size, demodulated
STYLE_ROWS = (0, 2, 2, 0)        # the latent row each layer reads: row 1 is read by nobody
STYLE_IDLE_D = 1                 # this demodulated layer's d takes no part in the loss


@pytest.mark.parametrize('N', [3, 33])
def test_style_mod_all_first_order(cuda_device, N):
    """hip_ops.style_mod_all (StyleModAllFn: seven grouped launches, a different Cin / Cout per group, ldx = 96) on four layers fed from
    one [N, 3, 32] latents tensor, against an fp64 evaluation of s = c_a y.A + b + 1, d = rsqrt(c_w^2 s^2.wsq + 1e-8) and its autograd,
    and against the per-layer hip_ops.style_mod on the same inputs: s, d and the gradients of A, b and w bit for bit (the same kernel
    instantiations on the same per-problem data), the latents' gradient to tolerance (autograd adds the layers' shares in its own order).
    Layer STYLE_IDLE_D's d is left out of the loss.  Autograd hands a Function a ZERO cotangent for an unused output, not None (neither
    Function turns that off), so the layer still runs its DEMOD_GRAD launches, on zeros: its filter gradient must be exactly zero (fp64
    has none) and its style gradient the plain gs."""
    from inclusivegan_amd import hip_ops
    from tests.util import rel_err
    D = 32
    rng = np.random.RandomState(1000 + N)
    lat = rng.randn(N, 3, D).astype(np.float32)
    par, cfg, gs, gd = [], [], [], []
    for Cin, Cout, k, demod in STYLE_LAYERS:
        par.append((rng.randn(D, Cin).astype(np.float32), (0.1 * rng.randn(Cin)).astype(np.float32), rng.randn(k, k, Cin, Cout).astype(np.float32)))
        cfg.append((float(1.0 / np.sqrt(D)), float(1.0 / np.sqrt(k * k * Cin)), demod))
        gs.append(rng.randn(N, Cin).astype(np.float32))
        gd.append(rng.randn(N, Cout).astype(np.float32))
    in_loss = [i for i, l in enumerate(STYLE_LAYERS) if l[3] and i != STYLE_IDLE_D]

    def grads(lat_t, tensors, outs, dt, dev):
        o = [s for s, _ in outs] + [outs[i][1] for i in in_loss]
        g = [torch.from_numpy(t).to(dt).to(dev) for t in gs] + [torch.from_numpy(gd[i]).to(dt).to(dev) for i in in_loss]
        ins = [lat_t] + [t for layer in tensors for t in layer]
        res = torch.autograd.grad(o, ins, g, allow_unused=True)
        return res[0], [res[1 + 3 * i:4 + 3 * i] for i in range(len(tensors))]

    # fp64
    lat64 = torch.from_numpy(lat).double().requires_grad_(True)
    t64 = [[torch.from_numpy(t).double().requires_grad_(True) for t in layer] for layer in par]
    o64 = []
    for i, (A, b, w) in enumerate(t64):
        c_a, c_w, demod = cfg[i]
        s = c_a * (lat64[:, STYLE_ROWS[i]] @ A) + b + 1.0
        o64.append((s, torch.rsqrt(c_w * c_w * ((s * s) @ (w * w).sum(dim=(0, 1))) + 1e-8) if demod else None))
    glat64, gpar64 = grads(lat64, t64, o64, torch.float64, 'cpu')

    def device_inputs():
        lat_t = torch.from_numpy(lat).to(cuda_device).requires_grad_(True)
        return lat_t, [[torch.from_numpy(t).to(cuda_device).requires_grad_(True) for t in layer] for layer in par]

    def layer_args(lat_t, tensors, i):
        A, b, w = tensors[i]
        y = lat_t[:, STYLE_ROWS[i]]
        assert y.stride(0) == 3 * D and hip_ops.style_mod_fusable(y, A, w, cfg[i][2])
        return dict(y=y, a_w=A, a_b=b, w=w, wsq=hip_ops.sumsq_taps_raw(w.detach()) if cfg[i][2] else None, c_a=cfg[i][0], c_w=cfg[i][1], demodulate=cfg[i][2])

    lat_a, t_a = device_inputs()
    o_all = hip_ops.style_mod_all([layer_args(lat_a, t_a, i) for i in range(len(par))])
    assert o_all is not None
    glat_a, gpar_a = grads(lat_a, t_a, o_all, torch.float32, cuda_device)
    lat_l, t_l = device_inputs()
    o_lay = [hip_ops.style_mod(**layer_args(lat_l, t_l, i)) for i in range(len(par))]
    glat_l, gpar_l = grads(lat_l, t_l, o_lay, torch.float32, cuda_device)

    fails, worst = [], {}

    def hold(name, got, want, bound):
        if want is None:      # a filter that reaches the loss through nothing
            if got is not None and float(got.abs().max()) != 0.0:
                fails.append((name, 'a gradient where fp64 has none'))
            return
        e = rel_err(got, want)
        key = name.split(' ')[0]
        worst[key] = (max(worst.get(key, (0.0, bound))[0], e), bound)
        if not e < bound:
            fails.append((name, e, bound))

    def same(name, a, b):
        if (a is None) != (b is None) or (a is not None and not torch.equal(a.view(torch.int32), b.view(torch.int32))):
            fails.append((name + ': grouped and per-layer results differ in bits', None if a is None or b is None else rel_err(a, b)))

    for i in range(len(par)):
        for j, (name, bound) in enumerate((('s', C.BOUND_FWD), ('d', C.BOUND_FWD))):
            if o64[i][j] is not None:
                hold('%s layer %d' % (name, i), o_all[i][j], o64[i][j], bound)
                hold('%s layer %d (per layer)' % (name, i), o_lay[i][j], o64[i][j], bound)
                same('%s layer %d' % (name, i), o_all[i][j], o_lay[i][j])
        for j, name in enumerate(('dA', 'db', 'dw')):
            hold('%s layer %d' % (name, i), gpar_a[i][j], gpar64[i][j], C.BOUND_GRAD)
            hold('%s layer %d (per layer)' % (name, i), gpar_l[i][j], gpar64[i][j], C.BOUND_GRAD)
            if gpar64[i][j] is not None:
                same('%s layer %d' % (name, i), gpar_a[i][j], gpar_l[i][j])
    hold('dlatents', glat_a, glat64, C.BOUND_GRAD)
    hold('dlatents (per layer)', glat_l, glat64, C.BOUND_GRAD)
    for g in (glat_a, glat_l):
        if float(g[:, 1].abs().max()) != 0.0:
            fails.append(('the unused latent row has a gradient',))
    _report('style_mod_all N %d' % N, {k: v[0] for k, v in worst.items()}, lambda key: worst[key][1])
    assert not fails, (len(fails), fails[:6])
