"""Host: (a) the fp64 restatement of tests/thin_cases.py is the convolution torch computes in fp64 (forward and the autograd weight gradient, both
filter layouts, scales, alpha, any pad / OH, stride 2 and up 2); (b) the library reports, for every row of every case table, the kernel the table
states, and plans the thin weight gradient's workspace the table expects (host-only calls, dummy pointers); (c) the inputs of
tests/test_gpu_thin_conv.py discriminate: an fp32 model of the kernels' own summation stays within a QUARTER of bound (a) on every case and of bound (b)
on every element of at least 12 terms (test_forward_inputs_discriminate says why not below, with the figures), and every mutant of the restatement in
FWD_MUTANTS / wgrad_mutants leaves a bound by a factor of 10 or more on at least one case of every table that targets its branch -- conditions on the
inputs, never fitted to a kernel's output; (d) thin shapes with bad arguments are refused with a reason
before anything reaches a device."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import thin_cases as C

A = 1 << 20      # a 16-byte-aligned address that is never dereferenced


def _lib():
    from inclusivegan_amd import _abi
    return _abi, _abi.get_plugin()


# ----------------------------------------------------------------------------- (a) the restatement against torch in fp64
def _torch_conv(c):
    """y and the autograd weight gradient for cotangent dy = ones * out-leaning values, in fp64, from torch.nn.functional.conv2d."""
    r = c.r
    x = torch.from_numpy(np.asarray(c.x, np.float64)).permute(0, 3, 1, 2)
    w = torch.from_numpy(np.asarray(c.w, np.float64))
    W = torch.flip(w, (0, 1)).permute(0, 1, 3, 2) if r.wt else w       # [k, k, Cin, Cout]
    W = W.clone().requires_grad_(True)
    if c.in_scale is not None:
        x = x * torch.from_numpy(np.asarray(c.in_scale, np.float64))[:, :, None, None]
    if r.up > 1:       # zeros between the pixels
        xu = torch.zeros(r.N, r.Cin, (r.H - 1) * r.up + 1, (r.W - 1) * r.up + 1, dtype=torch.float64)
        xu[:, :, ::r.up, ::r.up] = x
        x = xu
    y = torch.nn.functional.conv2d(x, W.permute(3, 2, 0, 1), stride=r.stride, padding=(r.pad_y, r.pad_x))
    assert y.shape[2:] == (r.OH, r.OW), (y.shape, r)
    if c.out_scale is not None:
        y = y * torch.from_numpy(np.asarray(c.out_scale, np.float64))[:, :, None, None]
    return c.alpha * c.gain * y.permute(0, 2, 3, 1), W


@pytest.mark.parametrize('row', [C.F('', 2, 5, 6, 64, 3, isc=1, osc=1), C.F('', 2, 5, 6, 64, 3, wt=1, isc=1), C.F('', 2, 5, 6, 8, 3, 3, wt=1, osc=1),
                                 C.F('', 2, 5, 6, 3, 16, 3, 2), C.F('', 2, 5, 6, 3, 16, 3, (0, 2), wt=1), C.F('', 2, 9, 7, 8, 3, 3, 0, 4, 3, stride=2),
                                 C.F('', 2, 4, 5, 8, 3, 3, 2, 9, 11, wt=1, up=2), C.F('', 1, 3, 20, 3, 16, 3, act=1)])
def test_restatement_is_torch_conv2d_in_fp64(row):
    c = C.fwd_case(row)
    want, _ = _torch_conv(c)
    y, S, T = c.ref
    assert C.rel_err64(y, want.detach().numpy()) < 1e-13
    assert (S >= np.abs(y) * (1 - 1e-12)).all() and 1 <= T.min() and T.max() <= row.k * row.k * row.Cin


@pytest.mark.parametrize('row', [C.G('', 'out', 2, 5, 6, 16, 3, 1), C.G('', 'in', 2, 5, 6, 16, 3, 1), C.G('', 'out', 3, 4, 3, 8, 2, isc=1, osc=1, k=3),
                                 C.G('', 'in', 3, 4, 3, 8, 4, k=3)])
def test_weight_gradient_restatement_is_the_autograd_gradient(row):
    c = C.wgrad_case(row)
    fc = SimpleNamespace(r=C.F('', row.N, row.H, row.W, c.Cin, c.Cout, row.k), x=c.x, w=np.zeros((row.k, row.k, c.Cin, c.Cout), np.float32),      # linear in the filter:
                         in_scale=c.in_scale, out_scale=c.out_scale, alpha=c.alpha, gain=1.0)                                                      # its value does not matter
    y, W = _torch_conv(fc)
    (y * torch.from_numpy(np.asarray(c.dy, np.float64))).sum().backward()
    dw, S, T = c.ref
    assert C.rel_err64(dw, W.grad.numpy()) < 1e-13
    assert (S >= np.abs(dw) * (1 - 1e-12)).all() and T.max() == row.N * row.H * row.W


def test_restatement_counts_the_terms_in_range():
    """T: nine taps inside, six on an edge, four in a corner (pad 1); S = |y| on all-positive operands."""
    x, w = np.ones((1, 4, 5, 2), np.float32), np.ones((3, 3, 2, 4), np.float32)
    y, S, T = C.conv(x, w, KH=3, KW=3, Cout=4, pad_y=1, pad_x=1, OH=4, OW=5, alpha=0.5)
    assert T[0, 0, 0, 0] == 8 and T[0, 0, 2, 0] == 12 and T[0, 1, 2, 0] == 18 and np.array_equal(y, S) and np.array_equal(y[..., 0], 0.5 * T[..., 0])
    assert C.ratio_b(y + C.bound_b(S, T) * 0.99, y, S, T) < 1.0 < C.ratio_b(y + C.bound_b(S, T) * 1.01, y, S, T)


# ----------------------------------------------------------------------------- (b) names and plans
def fwd_name(r):
    _abi, lib = _lib()
    p = _abi.Conv2DParams(**C.fwd_fields(r, lambda name, extra: A * (2 + 'x w y in_scale out_scale workspace'.split().index(name)) + 4 * extra))
    buf = ctypes.create_string_buffer(128)
    _abi.check(lib.igan_conv2d_kernel_name(ctypes.byref(p), buf, 128))
    return buf.value.decode()


def wgrad_name_and_plan(r):
    _abi, lib = _lib()
    c = SimpleCase(r)
    p = _abi.Conv2DWgradParams(**C.wgrad_fields(c, lambda name, extra: A * (2 + 'x dy dw in_scale out_scale workspace'.split().index(name)) + 4 * extra, (1, 0)))
    buf = ctypes.create_string_buffer(128)
    _abi.check(lib.igan_conv2d_wgrad_kernel_name(ctypes.byref(p), buf, 128))
    splits, floats = ctypes.c_int(0), ctypes.c_size_t(0)
    _abi.check(lib.igan_conv2d_wgrad_plan(ctypes.byref(p), ctypes.byref(splits), ctypes.byref(floats)))
    return buf.value.decode(), splits.value, floats.value


class SimpleCase:
    """What wgrad_fields needs of a case, without its tensors."""

    def __init__(self, r):
        self.r, self.pad = r, (r.k - 1) // 2
        self.Cin, self.Cout = (r.C, r.T) if r.orient == 'out' else (r.T, r.C)


FWD_TABLES = ['FWD_OUT1', 'FWD_OUT9', 'FWD_IN1', 'FWD_IN9', 'FWD_SLIDE', 'FWD_LEAVE']
WGRAD_TABLES = ['WGRAD_ROWS', 'WGRAD_SLAB', 'WGRAD_FALLBACK', 'WGRAD_LEAVE']


def test_library_reports_the_kernel_of_every_row():
    bad = []
    for table in FWD_TABLES:
        for r in getattr(C, table):
            name = fwd_name(r)
            if not (name.startswith(r.name) and not name.startswith('thin_') if table == 'FWD_LEAVE' else name == r.name):
                bad.append((table, r, name))
    for table in WGRAD_TABLES:
        for r in getattr(C, table):
            name, splits, floats = wgrad_name_and_plan(r)
            if name != r.name:
                bad.append((table, r, name))
            elif r.name == C.WGRAD and (splits, floats) != (2, C.wgrad_plan_floats(r)):
                bad.append((table, r, 'plan', splits, floats, C.wgrad_plan_floats(r)))
    assert not bad, (len(bad), bad[:6])


def test_tables_cover_what_they_claim():
    """The coverage the module text of thin_cases promises, counted."""
    o1, o9, i1, i9, sl = C.FWD_OUT1, C.FWD_OUT9, C.FWD_IN1, C.FWD_IN9, C.FWD_SLIDE
    for rows, thin in ((o1, 'Cout'), (o9, 'Cout'), (i1, 'Cin'), (i9, 'Cin')):
        assert {getattr(r, thin) for r in rows} == {1, 2, 3, 4} and {r.wt for r in rows} == {0, 1}
    assert {r.Cin for r in o1} == {64, 128, 256, 512} and {r.Cin for r in o9} == {64, 256} and {r.Cout for r in i1} == {16, 64, 256, 512}
    for Cout in (1, 2, 3, 4):
        assert {(r.isc, r.osc) for r in o1 if r.Cout == Cout} == set(C.SCALES)
    assert {(r.isc, r.osc) for r in o9} == set(C.SCALES) and {r.osc for r in i1} == {0, 1} == {r.osc for r in i9}
    npix = lambda r: r.N * r.OH * r.OW
    for Cin, step in ((64, 16), (128, 8), (256, 4), (512, 4)):
        n = {npix(r) for r in o1 if r.Cin == Cin}
        assert 1 in n and any(v % step == step - 1 and v < step for v in n) and any(v % step == 1 and v > step for v in n) and any(v > 28 * step // 4 for v in n), (Cin, n)
    for Cout, step in ((16, 16), (64, 4), (256, 1), (512, 1)):
        n = {npix(r) for r in i1 if r.Cout == Cout}
        assert 1 in n and max(n) > 7 * step and (step == 1 or (step - 1 in n and step + 1 in n)), (Cout, n)
    for rows in (o9, i9):
        assert {(r.pad_y, r.pad_x) for r in rows} >= {(1, 1), (0, 0), (2, 2), (0, 2)} and {r.OH - r.H for r in rows} >= {0, -2, 2}
    # the sliding kernel's three conditions, both sides of each
    slides = lambda r: r.k == 3 and r.Cin == 3 and r.Cout <= 256 and r.OW >= 16
    assert all(slides(r) for r in sl) and not any(slides(r) for r in i9)
    assert any(r.Cin == 3 and r.Cout <= 256 and r.OW == 15 for r in i9) and any(r.Cin == 3 and r.Cout == 512 and r.OW >= 16 for r in i9)
    assert any(r.Cin == 4 and r.Cout <= 256 and r.OW >= 16 for r in i9)
    assert {r.OW for r in sl} == {16, 17, 32, 33, 34, 35, 65} and {r.H for r in sl} == {1, 2, 5} and {r.pad_x for r in sl} == {0, 1, 2}
    assert {r.Cout for r in sl} == {16, 64, 256} and {r.N for r in sl} == {1, 3} and {(r.wt, r.osc) for r in sl} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for OW in (16, 17, 32, 33, 34, 35, 65):
        assert {(r.H, r.pad_x) for r in sl if r.OW == OW} == {(1, 1), (1, 2), (2, 1), (2, 2), (5, 0), (5, 1), (5, 2)}
    wg = C.WGRAD_ROWS
    assert {(r.orient, r.C, r.T, r.N * 1000 + r.H * r.W) for r in wg} == {(o, c, t, n) for o in ('out', 'in') for c in (16, 64, 256, 1024) for t in (1, 2, 3, 4)
                                                                        for n in (24001, 2063, 3129, 3200)}
    assert {(r.orient, r.isc or r.osc) for r in wg} == {('out', 0), ('out', 1), ('in', 0), ('in', 1)}
    assert C.wgrad_block_ends(3, 129) == [64, 128] and C.wgrad_block_ends(3, 200) == [66, 133, 199] and C.wgrad_block_ends(2, 63) == [62]
    assert C.wgrad_block_ends(1536, 1025) == [1024] and {r.ws for r in C.WGRAD_FALLBACK} == {'null', 'short', 'offset'}
    assert all(r.N * C.wgrad_bps(r.N, r.H * r.W) >= 3 for r in C.WGRAD_FALLBACK)


# ----------------------------------------------------------------------------- (c) the model and the mutants
def _sentinel(y, index):
    m = np.array(y)
    m[index] = float(C.SENTINEL)
    return m


def _slide_zero_column(kx, ox, ix, ok):
    """The first pixel of a run that is not the row's first reads a zero column on its left (the hand-over of the column buffers at x = 32, 64)."""
    return ix, ok & ~((kx == 0) & (ox % 32 == 0) & (ox > 0))


def _slide_stale_column(OW, W):
    def cols(kx, ox, ix, ok):
        """The pixels of a run's last trip of three that sit behind the `ox + 1 < x1` / `ox + 2 < x1` guards take the previous pixel's right column."""
        if kx != 2:
            return ix, ok
        x0 = ox - ox % 32
        last_trip = x0 + ((np.minimum(x0 + 32, OW) - x0 - 1) // 3) * 3
        stale = (ox > last_trip)
        ix = np.where(stale, ix - 1, ix)
        return ix, (ix >= 0) & (ix < W)
    return cols


def fwd_mutants(c, slide=False):
    """{name: y of the mutated restatement} for the mutants that apply to this case."""
    r = c.r
    y = c.ref[0]
    out = {'last pixel lost': _sentinel(y, (-1, -1, -1)), 'alpha dropped': C.fwd_of(c, alpha=1.0)[0]}
    if r.Cin >= 64:
        out['last channel quad lost'] = C.fwd_of(c, x=c.x[..., :-4], w=c.w[..., :-4] if r.wt else c.w[:, :, :-4], in_scale=None if c.in_scale is None else c.in_scale[:, :-4])[0]
        if r.Cin == 512:
            out['second channel block lost'] = C.fwd_of(c, x=c.x[..., :256], w=c.w[..., :256] if r.wt else c.w[:, :, :256], in_scale=None if c.in_scale is None else c.in_scale[:, :256])[0]
    else:
        out['last channel quad lost'] = _sentinel(y, (Ellipsis, slice(-4, None)))
        if r.Cout == 512:
            out['second channel block lost'] = _sentinel(y, (Ellipsis, slice(256, None)))
    if r.k == 3:
        out['border tap clamped instead of zero'] = C.fwd_of(c, clamp=True)[0]
    if r.wt and r.k == 3:
        out['no spatial flip under w_transposed'] = C.fwd_of(c, flip=False)[0]
    if r.wt and min(r.Cin, r.Cout) > 1:       # with one channel on a side the two layouts are the same bytes
        out['no channel swap under w_transposed'] = C.fwd_of(c, swap=False)[0]
    if r.isc and r.N > 1:
        out["sample 0's in_scale for every sample"] = C.fwd_of(c, in_scale=np.repeat(c.in_scale[:1], r.N, 0))[0]
    if r.osc and r.N > 1:
        out["sample 0's out_scale for every sample"] = C.fwd_of(c, out_scale=np.repeat(c.out_scale[:1], r.N, 0))[0]
    if r.Cout > 1:
        co = np.arange(r.Cout) ^ 1
        out['output channels co and co ^ 1 exchanged'] = y[..., np.where(co < r.Cout, co, np.arange(r.Cout))]
    if slide:
        if r.OW > 32:
            out['sliding: zero column after a run boundary'] = C.fwd_of(c, cols=_slide_zero_column)[0]
        if any((min(x0 + 32, r.OW) - x0) % 3 != 1 for x0 in range(0, r.OW, 32)):
            out['sliding: stale column in the last pixels of a run'] = C.fwd_of(c, cols=_slide_stale_column(r.OW, r.W))[0]
    return out


def _exceeds(m, ref):
    """By how much a mutant leaves the looser-fitting of the two bounds: max(rel_err / (a), worst element / (b))."""
    y, S, T = ref
    return max(C.rel_err64(m, y) / C.BOUND_A, C.ratio_b(m, y, S, T))


FWD_MUTANTS = {      # table -> the mutants that must leave a bound by 10x on at least one of its cases
    'FWD_OUT1': {'last pixel lost', 'alpha dropped', 'last channel quad lost', 'second channel block lost', 'no channel swap under w_transposed',
                 "sample 0's in_scale for every sample", "sample 0's out_scale for every sample", 'output channels co and co ^ 1 exchanged'},
    'FWD_OUT9': {'last pixel lost', 'alpha dropped', 'last channel quad lost', 'border tap clamped instead of zero', 'no spatial flip under w_transposed',
                 'no channel swap under w_transposed', "sample 0's in_scale for every sample", "sample 0's out_scale for every sample",
                 'output channels co and co ^ 1 exchanged'},
    'FWD_IN1': {'last pixel lost', 'alpha dropped', 'last channel quad lost', 'second channel block lost', 'no channel swap under w_transposed',
                "sample 0's out_scale for every sample", 'output channels co and co ^ 1 exchanged'},
    'FWD_IN9': {'last pixel lost', 'alpha dropped', 'last channel quad lost', 'second channel block lost', 'border tap clamped instead of zero',
                'no spatial flip under w_transposed', 'no channel swap under w_transposed', "sample 0's out_scale for every sample",
                'output channels co and co ^ 1 exchanged'},
    'FWD_SLIDE': {'last pixel lost', 'alpha dropped', 'last channel quad lost', 'border tap clamped instead of zero', 'no spatial flip under w_transposed',
                  'no channel swap under w_transposed', "sample 0's out_scale for every sample", 'output channels co and co ^ 1 exchanged',
                  'sliding: zero column after a run boundary', 'sliding: stale column in the last pixels of a run'},
    'FWD_LEAVE': {'last pixel lost', 'alpha dropped'},
}


QUARTER_FROM_T = 12


def _model_shares(c):
    """The fp32 model against the two bounds: (share of (a), largest share of (b) among the elements with T >= QUARTER_FROM_T, largest share of (b) among the others,
    largest |model - ref| / ((T + 2 + [in_scale]) 2^-24 S): the model's own count of roundings, which no element may exceed)."""
    y, S, T = c.ref
    m = C.fwd_model32(c)
    err = np.abs(m.astype(np.float64) - y)
    Tb = np.broadcast_to(T, y.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        share = np.where(Tb > 0, err / C.bound_b(S, T), np.where(err == 0, 0.0, np.inf))
        own = np.where(Tb > 0, err / ((Tb + 2 + c.r.isc + c.r.act) * C.EPS24 * S), 0.0)
    big = Tb >= QUARTER_FROM_T
    return C.rel_err64(m, y) / C.BOUND_A, float(share[big].max()) if big.any() else 0.0, float(share[~big].max()) if (~big).any() else 0.0, float(own.max())


@pytest.mark.parametrize('table', FWD_TABLES)
def test_forward_inputs_discriminate(table):
    """The model: within a quarter of (a) on every case, and within a quarter of (b) on every element with at least QUARTER_FROM_T = 12 terms -- every element of a thin-output
    layer and of a 3x3 layer from 3 or 4 channels under SAME padding (corners 12 or 16 terms, edges 18 or 24, inside 27 or 36).  Below that a quarter of (b) is not there to
    be had, by counting: the fused multiply-add chain makes T roundings, alpha and out_scale one each, every one of them up to 2^-24 of S, against a quarter of 1.01 (T + 4);
    the 1x1 layers from 1 ... 4 channels and the one-tap corners under pad 2 measure 0.47, 0.42, 0.39, 0.36 of (b) at T = 1, 2, 3, 4, 0.33 at 6 and 0.29 at 9 on these
    inputs (0.25 at 12 and 18, 0.18 at 27, 0.03 at 64), whatever the pixel count.  Those elements are held to the model's own count of roundings instead, which checks S
    and T of the restatement; on the device they are held to (b) itself like every other."""
    worst = [0.0, 0.0, 0.0, 0.0]
    best, hits, bad = {}, {}, []
    for r in getattr(C, table):
        c = C.fwd_case(r)
        sh = _model_shares(c)
        worst = [max(a, b) for a, b in zip(worst, sh)]
        if not (sh[0] < 0.25 and sh[1] < 0.25 and sh[3] <= 1.0):
            bad.append(('model', r) + sh)
        for name, mut in fwd_mutants(c, table == 'FWD_SLIDE').items():
            e = _exceeds(mut, c.ref)
            best[name] = max(best.get(name, 0.0), e)
            hits[name] = [hits.get(name, [0, 0])[0] + (e >= 10.0), hits.get(name, [0, 0])[1] + 1]
    print('%-9s fp32 model at most %.3f of (a), %.3f of (b) at T >= %d, %.3f of (b) below, %.3f of its own roundings; mutants (largest x bound, cases at 10x or more): %s'
          % (table, worst[0], worst[1], QUARTER_FROM_T, worst[2], worst[3], ', '.join('%s %.0f %d/%d' % (k, min(best[k], 1e9), hits[k][0], hits[k][1]) for k in sorted(best))))
    assert not bad, (len(bad), bad[:6])
    assert FWD_MUTANTS[table] <= set(best), FWD_MUTANTS[table] - set(best)
    assert all(best[k] >= 10.0 for k in FWD_MUTANTS[table]), {k: best[k] for k in FWD_MUTANTS[table] if best[k] < 10.0}


def wgrad_mutants(c):
    r = c.r
    dw = c.ref[0]
    HW = r.H * r.W
    wide_axis = 2 if r.orient == 'out' else 3
    keep = lambda pix: np.where(np.isin(np.arange(HW), pix), 0.0, 1.0)[None, :].repeat(r.N, 0).reshape(r.N, r.H, r.W)
    last = np.ones((r.N, r.H, r.W))
    last[-1, -1, -1] = 0.0
    quad = [slice(None)] * 4
    quad[wide_axis] = slice(-4, None)
    out = {'last pixel lost': C.wgrad_of(c, last)[0], 'alpha dropped': C.wgrad_of(c, alpha=1.0)[0], 'last channel quad lost': _sentinel(dw, tuple(quad)),
           'last pixel of every block lost': C.wgrad_of(c, keep(C.wgrad_block_ends(r.N, HW)))[0]}
    if r.T > 1:
        t = np.arange(r.T) ^ 1
        t = np.where(t < r.T, t, np.arange(r.T))
        out['thin channels t and t ^ 1 exchanged'] = dw[:, :, :, t] if r.orient == 'out' else dw[:, :, t, :]
    if r.N > 1 and (r.isc or r.osc):
        out["sample 0's scale for every sample"] = C.wgrad_of(c, **{k: None if getattr(c, k) is None else np.repeat(getattr(c, k)[:1], r.N, 0) for k in ('in_scale', 'out_scale')})[0]
    if -(-HW // C.wgrad_bps(r.N, HW)) > 1024:
        out['second slab lost'] = C.wgrad_of(c, keep(np.arange(1024, HW)))[0]      # one block per sample in every such row
    return out


@pytest.mark.parametrize('table', ['WGRAD_ROWS', 'WGRAD_SLAB', 'WGRAD_FALLBACK'])
def test_weight_gradient_inputs_discriminate(table):
    worst_a = worst_b = 0.0
    best, bad = {}, []
    for r in getattr(C, table):
        c = C.wgrad_case(r)
        dw, S, T = c.ref
        m = C.wgrad_model32(c)
        ra, rb = C.rel_err64(m, dw) / C.BOUND_A, C.ratio_b(m, dw, S, T)
        worst_a, worst_b = max(worst_a, ra), max(worst_b, rb)
        if not ra < 0.25:
            bad.append(('model', r, ra))
        for name, mut in wgrad_mutants(c).items():
            e = C.rel_err64(mut, dw) / C.BOUND_A
            best[name] = max(best.get(name, 0.0), e)
            if name in ('last pixel of every block lost', 'second slab lost') and not e >= 10.0:       # these two on EVERY case they apply to
                bad.append((name, r, e))
    print('%-14s fp32 model at most %.3f of (a) (%.2e of (b), not held); mutants (largest x (a)): %s'
          % (table, worst_a, worst_b, ', '.join('%s %.0f' % (k, min(best[k], 1e9)) for k in sorted(best))))
    assert not bad, (len(bad), bad[:6])
    need = {'last pixel of every block lost', 'alpha dropped', 'last channel quad lost'} | ({'second slab lost'} if table == 'WGRAD_SLAB' else
                                                                                          {'last pixel lost', 'thin channels t and t ^ 1 exchanged', "sample 0's scale for every sample"})
    assert need <= set(best) and all(best[k] >= 10.0 for k in need), {k: best.get(k) for k in need}


# ----------------------------------------------------------------------------- (d) refusals
def _refused(rc, needle, code=None):
    _abi, lib = _lib()
    msg = lib.igan_last_error()
    assert rc == (code or _abi.IGAN_ERR_INVALID_ARGUMENT) and needle.encode() in msg, (rc, needle, msg)


def test_thin_shapes_with_bad_arguments_are_refused():
    """Every geometry error of fwd_geometry_check that a thin shape can carry, through the three entry points that share the check; NULL stream, dummy pointers:
    nothing here may launch.  A thin shape with a noise operand and act == 0 never reaches the thin-channel launch: the geometry check, which every entry point
    runs first, refuses it (noise belongs to the fused epilogue, and a call with act != 0 is not a thin one)."""
    _abi, lib = _lib()
    thin_out, thin_in = C.F(C.OUT1, 2, 4, 4, 64, 3), C.F(C.IN9, 2, 4, 16, 3, 64, 3)
    assert fwd_name(thin_out) == C.OUT1 and fwd_name(thin_in) == C.IN9
    cases = []
    for r in (thin_out, thin_in):
        cases += [(r, dict(x=None), 'conv2d: null buffer'), (r, dict(w=None), 'conv2d: null buffer'), (r, dict(y=None), 'conv2d: null buffer'),
                  (r, dict(N=0), 'input dims must be positive'), (r, dict(H=0), 'input dims must be positive'),
                  (r, dict(OH=0), 'output dims must be positive'), (r, dict(OW=-1), 'output dims must be positive'),
                  (r, dict(noise=A), 'noise needs the fused epilogue'), (r, dict(noise=A, noise_strength=A), 'noise needs the fused epilogue')]
    cases += [(thin_out, dict(N=1 << 16, H=128, W=128, OH=128, OW=128), 'input too large'),
              (C.F(C.IN1, 1, 1, 1, 1, 512), dict(N=1 << 9, H=1 << 7, W=1 << 7, OH=1 << 7, OW=1 << 7), 'output too large')]
    for r, over, why in cases:
        fields = C.fwd_fields(r, lambda name, extra: A)
        fields.update(over)
        p = _abi.Conv2DParams(**fields)
        buf = ctypes.create_string_buffer(128)
        s, t, f = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
        _refused(lib.igan_conv2d(None, ctypes.byref(p)), why)
        _refused(lib.igan_conv2d_kernel_name(ctypes.byref(p), buf, 128), why)
        _refused(lib.igan_conv2d_plan(ctypes.byref(p), ctypes.byref(s), ctypes.byref(t), ctypes.byref(f)), why)
