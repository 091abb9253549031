"""GPU: every form of the thin-channel convolution kernels (csrc/thin_conv.hip) at the C ABI against the fp64 restatement of tests/thin_cases.py, at
the smallest shapes that reach each branch (the tables of thin_cases name them): thin_out_kernel<1> / <9> at 16, 32 and 64 lanes per pixel and two
channel blocks, Cout 1 ... 4, both filter layouts, every combination of scales, one pixel, ragged and repeated trips, pads 0 / 1 / 2 with OH following;
thin_in_kernel<1> / <9> at Cin 1 ... 4 and 4 ... 64 lanes per pixel; the sliding-window kernel of Cin = 3 at run tails of 1, 2 and 3 pixels, one to three
runs per row and all-border inputs; thin_wgrad_kernel at 4 ... 256 lanes per pixel, one to three workgroups per sample with ragged last ones, the
second 1024-pixel slab, and the launch-time fallbacks to the tile kernels; and shapes that must leave the family and still be right.

The structs are built here from _abi.Conv2DParams / Conv2DWgradParams.  Every operand, output and workspace of a launch lies in ONE flat device
buffer between 64-float guard bands of a finite sentinel (dense_cases.Arena); outputs and workspaces start as the sentinel.  After each launch every guard
float and every input must be unchanged, every output element finite and written, and the library, asked with the real pointers, must name the kernel
the table states.  Bounds (thin_cases): (a) tests.util.rel_err < 3e-5; (b) per element |got - ref| <= 1.01 (T + 4) 2^-24 S -- asserted for the forward
and data-gradient cases, printed for the weight gradients, which run twice and must repeat bit for bit.  A test loops over its rows, collects every
failure, prints its largest (a) and (b) per kernel, then asserts."""
import ctypes
import time

import numpy as np
import pytest

import thin_cases as C
from test_gpu_dense_small import Launch, _bits_equal, _stream
from tests.util import rel_err

pytestmark = pytest.mark.gpu

DUMMY = 1 << 20      # a 16-byte-aligned address for the host-only planning calls


def _dummy(names):
    return lambda name, extra: DUMMY * (2 + names.index(name)) + 4 * extra


def _report(title, worst):
    for name in sorted(worst):
        a, b = worst[name]
        print('%-16s %-34s largest (a) rel_err %.3e of %.0e   largest (b) %.3f of the bound%s' % (title, name, a, C.BOUND_A, b, '' if title.startswith('forward') else ' (not held)'))


# ----------------------------------------------------------------------------- forward and data gradient
def _fwd_call(p):
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    return lambda: lib.igan_conv2d(_stream(), ctypes.byref(p))


def _fwd_name(p):
    from inclusivegan_amd import _abi
    buf = ctypes.create_string_buffer(128)
    _abi.check(_abi.get_plugin().igan_conv2d_kernel_name(ctypes.byref(p), buf, 128))
    return buf.value.decode()


def _fwd_plan(p):
    from inclusivegan_amd import _abi
    s, t, f = ctypes.c_int(1), ctypes.c_int(0), ctypes.c_size_t(0)
    _abi.check(_abi.get_plugin().igan_conv2d_plan(ctypes.byref(p), ctypes.byref(s), ctypes.byref(t), ctypes.byref(f)))
    return s.value, t.value, f.value


@pytest.mark.parametrize('table', ['FWD_OUT1', 'FWD_OUT9', 'FWD_IN1', 'FWD_IN9', 'FWD_SLIDE', 'FWD_LEAVE'])
def test_forward(cuda_device, table):
    from inclusivegan_amd import _abi
    fails, worst, t0 = [], {}, time.time()
    for r in getattr(C, table):
        c = C.fwd_case(r)
        y64, S, T = c.ref
        plan = _fwd_plan(_abi.Conv2DParams(**C.fwd_fields(r, _dummy('x w y in_scale out_scale workspace'.split()))))
        arena = C.Arena()
        C.place_fwd(arena, c, plan[2])
        L = Launch(arena, cuda_device)
        p = _abi.Conv2DParams(**C.fwd_fields(r, lambda name, extra: arena.addr(L.base, name, extra), plan))
        name = _fwd_name(p)
        if not (name.startswith(r.name) and not name.startswith('thin_') if table == 'FWD_LEAVE' else name == r.name):
            fails.append((r, 'runs on %s' % name))
        if _fwd_plan(p) != plan:
            fails.append((r, 'the plan changes with the real pointers', plan, _fwd_plan(p)))
        fails += [(r, b) for b in L.run(_fwd_call(p))]
        y = arena.out(L.after, 'y')
        if not np.isfinite(y).all() or (y == C.SENTINEL).any():
            fails.append((r, 'y has %d elements that are not finite or were never written' % int((~np.isfinite(y) | (y == C.SENTINEL)).sum())))
            continue
        a, b = rel_err(y, np.array(y64)), C.ratio_b(y, y64, S, T)
        key = name if table != 'FWD_LEAVE' else name.split('<')[0]
        worst[key] = (max(worst.get(key, (0.0, 0.0))[0], a), max(worst.get(key, (0.0, 0.0))[1], b))
        if not a < C.BOUND_A:
            fails.append((r, '(a)', a, C.BOUND_A))
        if not b <= 1.0:
            fails.append((r, '(b): an element is at %.3f of its bound' % b))
    _report('forward %s' % table[4:], worst)
    print('%d launches in %.1f s' % (len(getattr(C, table)), time.time() - t0))
    assert not fails, (len(fails), fails[:6])


# ----------------------------------------------------------------------------- weight gradient
WG_NAMES = 'x dy dw in_scale out_scale workspace'.split()


def _wgrad_plan_and_name(p):
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    s, f = ctypes.c_int(1), ctypes.c_size_t(0)
    _abi.check(lib.igan_conv2d_wgrad_plan(ctypes.byref(p), ctypes.byref(s), ctypes.byref(f)))
    buf = ctypes.create_string_buffer(128)
    _abi.check(lib.igan_conv2d_wgrad_kernel_name(ctypes.byref(p), buf, 128))
    return (s.value, f.value), buf.value.decode()


def _wgrad_once(dev, c, plan, fails):
    """One launch into a fresh arena.  -> (Launch, the library's kernel name for the real pointers)."""
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    arena = C.Arena()
    C.place_wgrad(arena, c, plan[1])
    L = Launch(arena, dev)
    p = _abi.Conv2DWgradParams(**C.wgrad_fields(c, lambda name, extra: arena.addr(L.base, name, extra), plan))
    _, name = _wgrad_plan_and_name(p)
    fails += [(c.r, b) for b in L.run(lambda: lib.igan_conv2d_wgrad(_stream(), ctypes.byref(p)))]
    return L, name


def _workspace_story(c, L):
    """What the workspace tells about the kernel that ran.  The thin kernel fills one [C][4] partial per workgroup; the tile kernels, split in two, fill two
    partial filters at the address they were given and nothing behind them."""
    r = c.r
    if r.ws == 'null' or 'workspace' not in L.arena.spans:
        return []
    ws = L.arena.out(L.after, 'workspace')
    written = ws != C.SENTINEL
    thin_floats = r.N * C.wgrad_bps(r.N, r.H * r.W) * r.C * 4
    if r.ws == 'plan':
        return [] if r.name != C.WGRAD or written[:thin_floats].all() else ['the thin kernel left %d of its %d partial sums unwritten' % (int((~written[:thin_floats]).sum()), thin_floats)]
    lead = 1 if r.ws == 'offset' else 0
    tile_floats = 2 * r.C * r.T
    assert tile_floats < thin_floats - 1
    bad = []
    if written[:lead].any() or written[lead + tile_floats:].any():
        bad.append('the call did not fall back to the tile kernels: %d workspace floats outside their two partial filters were written' % int(written[:lead].sum() + written[lead + tile_floats:].sum()))
    if not written[lead:lead + tile_floats].all():
        bad.append('the tile kernels left partial filters unwritten')
    return bad


WG_PARAMS = [('WGRAD_ROWS', 16), ('WGRAD_ROWS', 64), ('WGRAD_ROWS', 256), ('WGRAD_ROWS', 1024), ('WGRAD_SLAB', 0), ('WGRAD_FALLBACK', 0), ('WGRAD_LEAVE', 0)]


@pytest.mark.parametrize('table,C_', WG_PARAMS, ids=['%s%s' % (t, '-C%d' % c if c else '') for t, c in WG_PARAMS])
def test_weight_gradient(cuda_device, table, C_):
    from inclusivegan_amd import _abi
    fails, worst, t0 = [], {}, time.time()
    rows = [r for r in getattr(C, table) if not C_ or r.C == C_]
    for r in rows:
        c = C.wgrad_case(r)
        dw64, S, T = c.ref
        plan, _ = _wgrad_plan_and_name(_abi.Conv2DWgradParams(**C.wgrad_fields(c, _dummy(WG_NAMES), (1, 0))))      # planned without a workspace, as a caller does
        if r.name == C.WGRAD and plan != (2, C.wgrad_plan_floats(r)):
            fails.append((r, 'plan', plan, C.wgrad_plan_floats(r)))
            continue
        runs = []
        for _ in range(2):
            L, name = _wgrad_once(cuda_device, c, plan, fails)
            if name != r.name:
                fails.append((r, 'runs on %s' % name))
            fails += [(r, b) for b in _workspace_story(c, L)]
            runs.append(L.arena.out(L.after, 'dw'))
        dw = runs[0]
        if not _bits_equal(runs[0], runs[1]):
            fails.append((r, 'two runs differ', C.rel_err64(runs[1], runs[0])))
        if not np.isfinite(dw).all() or (dw == C.SENTINEL).any():
            fails.append((r, 'dw has elements that are not finite or were never written'))
            continue
        a, b = rel_err(dw, np.array(dw64)), C.ratio_b(dw, dw64, S, T)
        key = '%s%s' % (r.name, '' if r.ws == 'plan' else ', workspace %s' % r.ws)
        worst[key] = (max(worst.get(key, (0.0, 0.0))[0], a), max(worst.get(key, (0.0, 0.0))[1], b))
        if not a < C.BOUND_A:
            fails.append((r, '(a)', a, C.BOUND_A))
    _report('wgrad %s' % table[6:], worst)
    print('%d rows, two launches each, in %.1f s' % (len(rows), time.time() - t0))
    assert not fails, (len(fails), fails[:6])
