"""Non-finite propagation cases: case tables, fp64 oracles and the shared assertions (plain Python: NumPy / PyTorch on the CPU, no GPU import).

A case takes an op at an existing small test shape with finite inputs, poisons ONE element of one input with NaN, +inf or -inf, and names
  outputs      what the op returns (forward results and gradients),
  oracle       the same operation in fp64 on the CPU (oracle/ functions, or the _conv_oracle formulation of tests/test_gpu_ops.py),
  unreachable  per output, the elements the poison cannot reach (other samples, other channels, other groups, windows that miss it),
  reach        per output, where the HIP result may be non-finite although the oracle is finite (declared, see below); None = nowhere,
  mask_only    outputs that are checked like scalars (assertions 1, 2 and 4, no values): the poison reaches more than a quarter of them
               BY CONSTRUCTION at the shapes the cases are set at -- an in_scale entry poisons a whole sample of a batch of 1..3 (y, and the
               per-sample rows of ModConv2dFn's ds / dd), a 3-channel side of a thin convolution is a third of the tensor, the three distances
               of the LPIPS case hold the poisoned one, a NaN in the style path's A reaches every d, the cotangent of the minibatch-stddev
               statistic reaches every element of its group (half the batch).  test_nonfinite_cases.py requires that every output NOT listed
               here keeps >= 75 % of its elements finite in the oracle, and that a listed one does not.

check_outputs() is the contract (DESIGN.md "Non-finite values"):
  1. no laundering: oracle non-finite => HIP non-finite (NaN and +-inf are not told apart: the piece form turns inf into NaN);
  2. no spreading: on `unreachable` the HIP result on the poisoned input is bit-identical to the HIP result on the clean input;
  3. values: where both are finite they agree to the tolerance of the op's existing test in tests/test_gpu_ops.py, normalised over the
     jointly finite elements;
  4. HIP non-finite where the oracle is finite only inside the declared `reach`.
The oracle's non-finite set is taken in the output's number format (fp32): an fp64 value beyond FLT_MAX counts as non-finite.

Contracts that are the reference kernel's and not the framework's (stated here once, used by every case with a select-based activation):
relu(NaN) = 0, relu(-inf) = 0, lrelu(NaN) = NaN; the gradient forms select on ref = y / gain the same way (ref = NaN takes the `else` arm).
The oracle for these is oracle.fused_bias_act.fused_bias_act_kernel_ref (the restated select), never torch.relu.

Declared reaches:
  * zero-extended FIR (upfirdn2d fast path with fewer than 4x4 taps): a 4x4 footprint -- input (iy, ix) reaches outputs
    oy in [iy + pad0 - 3, iy + pad0], ox likewise, same sample, same channel (0 * inf = NaN on the extra taps);
  * piece form of the convolutions: the poisoned element's scale group -- the pixel (all channels) for the forward / data-gradient row image,
    the channel (all pixels) for the weight gradient's column image, the output channel (all taps and input channels) for the filter image.
    With the poison at an interior pixel / the centre tap, every member of the group meets the poison in the oracle too, so the reach equals the
    oracle's own set there; a border pixel is recorded (profiles/nonfinite.txt), not asserted.
"""
import numpy as np
import torch
import torch.nn.functional as F

KINDS = {'nan': np.float32(np.nan), '+inf': np.float32(np.inf), '-inf': np.float32(-np.inf)}
FLT_MAX = float(np.finfo(np.float32).max)


def nonfinite32(t):
    """Non-finite set of an fp64 result in the output's format (fp32)."""
    return ~torch.isfinite(torch.as_tensor(t).detach().to(torch.float64).to(torch.float32))


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).double()


class Case:
    def __init__(self, op, cfg, name, make, poison, oracle, unreachable, tol, reach=None, mask_only=(), exact_mask=False, path='', may_vanish=False):
        self.op, self.cfg, self.name, self.make, self.poison, self.oracle = op, cfg, name, make, poison, oracle
        self.unreachable, self.tol, self.reach, self.mask_only, self.exact_mask, self.path = unreachable, tol, reach, tuple(mask_only), exact_mask, path
        self.may_vanish = may_vanish      # relu's select turns NaN and -inf into 0 (the reference kernel's formula): the oracle may hold no non-finite value at all

    @property
    def id(self):
        inp, idx, kind = self.poison
        return '%s-%s-%s%s-%s' % (self.op, self.name, inp, ''.join('_%d' % i for i in idx), kind)

    def inputs(self, poisoned):
        d = {k: np.array(v, dtype=np.float32, copy=True) for k, v in self.make().items()}
        if poisoned:
            inp, idx, kind = self.poison
            assert np.isfinite(d[inp][idx])
            d[inp][idx] = KINDS[kind]
        return d

    def want(self, poisoned=True):
        return self.oracle(self.cfg, {k: t64(v) for k, v in self.inputs(poisoned).items()})

    def masks(self, shapes):
        """(unreachable, reach) boolean arrays per output name."""
        un = self.unreachable(self.cfg, self.poison, shapes)
        rc = self.reach(self.cfg, self.poison, shapes) if self.reach is not None else {}
        return un, rc


def check_oracle_side(case):
    """The condition on the cases (CPU, oracle only): clean inputs give finite results, every output that is checked for values keeps >= 75 % of its
    elements finite, a mask_only output does not (so nothing dodges the value check), the unreachable set is finite and equals the clean result."""
    clean = case.want(False)
    want = case.want(True)
    shapes = {k: tuple(v.shape) for k, v in want.items()}
    un, rc = case.masks(shapes)
    hit = False
    for name, w in want.items():
        assert bool(torch.isfinite(clean[name]).all()), (case.id, name, 'clean oracle not finite')
        bad = nonfinite32(w)
        hit |= bool(bad.any())
        frac = 1.0 - float(bad.double().mean())
        if w.dim() > 0 and w.numel() > 1:
            if name in case.mask_only:
                assert frac < 0.75, (case.id, name, frac, 'listed as mask_only although the value check would see >= 75 %')
            else:
                assert frac >= 0.75, (case.id, name, frac)
        if name in un:
            m = torch.from_numpy(np.broadcast_to(un[name], shapes[name]).copy())
            assert not bool(bad[m].any()), (case.id, name, 'unreachable set is not finite in the oracle')
            assert torch.equal(w[m], clean[name][m]), (case.id, name, 'unreachable set depends on the poison in the oracle')
        if name in rc:
            r = torch.from_numpy(np.broadcast_to(rc[name], shapes[name]).copy())
            if name in un:
                assert not bool((r & m).any()), (case.id, name, 'declared reach overlaps the unreachable set')
    assert hit or case.may_vanish, (case.id, 'the poison reaches no output in the oracle')


def check_outputs(case, want, got, got_clean):
    """Assertions 1-4 of the module docstring for every output; returns one report line per output."""
    shapes = {k: tuple(v.shape) for k, v in want.items()}
    un, rc = case.masks(shapes)
    lines = []
    for name, w in want.items():
        g = got[name].detach().cpu()
        gc = got_clean[name].detach().cpu()
        assert tuple(g.shape) == shapes[name], (case.id, name, g.shape, shapes[name])
        o_bad = nonfinite32(w)
        h_bad = ~torch.isfinite(g)
        reach = torch.from_numpy(np.broadcast_to(rc[name], shapes[name]).copy()) if name in rc else torch.zeros(shapes[name], dtype=torch.bool)
        extra = h_bad & ~o_bad
        laundered = o_bad & ~h_bad
        where = 'none' if not bool(extra.any()) else ('inside the declared reach' if not bool((extra & ~reach).any()) else 'OUTSIDE the declared reach')
        lines.append('NONFINITE %-10s %-34s %-28s poison %-8s at %s[%s]  %-4s oracle %6d  hip %6d  laundered %d  extra %d (%s)  of %d' % (
            case.op, case.name, case.path, case.poison[2], case.poison[0], ','.join(str(i) for i in case.poison[1]), name,
            int(o_bad.sum()), int(h_bad.sum()), int(laundered.sum()), int(extra.sum()), where, w.numel()))
        print(lines[-1])
        assert bool(torch.isfinite(gc).all()), (case.id, name, 'HIP result on the clean input is not finite')
        assert not bool(laundered.any()), (case.id, name, 'laundered', int(laundered.sum()), torch.nonzero(laundered)[:4].tolist())                     # 1
        if name in un:                                                                                                                                  # 2
            m = torch.from_numpy(np.broadcast_to(un[name], shapes[name]).copy())
            assert torch.equal(g[m].view(torch.int32), gc[m].view(torch.int32)), (case.id, name, 'spread into the unreachable set',
                                                                                  int((g[m].view(torch.int32) != gc[m].view(torch.int32)).sum()))
        assert not bool((extra & ~reach).any()), (case.id, name, 'non-finite outside the declared reach', torch.nonzero(extra & ~reach)[:4].tolist())   # 4
        if case.exact_mask:
            assert torch.equal(h_bad, o_bad), (case.id, name, 'mask differs from the oracle')
        if w.dim() > 0 and w.numel() > 1 and name not in case.mask_only:                                                                                # 3
            both = ~o_bad & ~h_bad
            err = float((g.double()[both] - w[both]).abs().max() / (w[both].abs().max() + 1e-30))
            tol = case.tol[name] if isinstance(case.tol, dict) else case.tol
            assert err < tol, (case.id, name, err, tol)
    return lines


def _other(shape, axis, index):
    """True everywhere except at `index` along `axis`."""
    m = np.ones(shape, dtype=bool)
    sl = [slice(None)] * len(shape)
    sl[axis] = index
    m[tuple(sl)] = False
    return m


def _all(shape):
    return np.ones(shape, dtype=bool)


def _kernel_ref(x, ref, grad, act_idx, alpha, gain):
    from oracle.fused_bias_act import fused_bias_act_kernel_ref
    return fused_bias_act_kernel_ref(x, None, ref, grad, act_idx, alpha, gain, 1).reshape(x.shape)


# ----------------------------------------------------------------------------- bias + noise + activation epilogue
BAN_ACTS = {'lrelu': (3, 0.2, float(np.sqrt(2))), 'linear': (1, 0.0, 1.0), 'relu': (2, 0.0, float(np.sqrt(2)))}
BAN_STRENGTH = 0.37


def ban_make(shape):
    def make():
        rng = np.random.RandomState(len(shape) * 31 + shape[1])
        n, c, h, w = shape
        x = rng.randn(*shape)
        x[0, 5, h - 1, w - 2] = 6.0       # where dy is poisoned the unit is active: relu's gradient select would drop the poison otherwise
        return dict(x=x, b=rng.randn(c), noise=rng.randn(n, 1, h, w), dy=rng.randn(*shape))
    return make


def ban_oracle(cfg, t):
    """y = act(x + noise * strength + b) * gain with the reference kernel's selects; dx = act'(ref = y) dy; db, dstrength its sums."""
    shape, act = cfg
    idx, alpha, gain = BAN_ACTS[act]
    pre = t['x'] + t['noise'] * BAN_STRENGTH + t['b'].view(1, -1, 1, 1)
    y = _kernel_ref(pre, None, 0, idx, alpha, gain)
    dx = _kernel_ref(t['dy'], y, 1, idx, alpha, gain)
    return dict(y=y, dx=dx, db=dx.sum(dim=(0, 2, 3)), ds=(dx * t['noise']).sum())


def ban_unreachable(cfg, poison, shapes):
    inp, idx, _ = poison
    s = shapes['y']
    if inp == 'x':
        return dict(y=_other(s, 0, idx[0]), dx=_other(s, 0, idx[0]), db=_other(shapes['db'], 0, idx[1]))
    if inp == 'noise':      # the select of the gradient form sees the poisoned pixel of every channel: no channel of db is out of reach
        return dict(y=_other(s, 0, idx[0]), dx=_other(s, 0, idx[0]))
    if inp == 'b':
        return dict(y=_other(s, 1, idx[0]), dx=_other(s, 1, idx[0]), db=_other(shapes['db'], 0, idx[0]))
    return dict(y=_all(s), dx=_other(s, 0, idx[0]), db=_other(shapes['db'], 0, idx[1]))      # dy


def ban_cases():
    out = []
    for shape in [(2, 8, 5, 6), (3, 128, 17, 9)]:
        n, c, h, w = shape
        for act in ('lrelu', 'linear', 'relu'):
            for inp, idx in (('x', (1, c - 3, h - 2, 1)), ('noise', (n - 1, 0, 2, w - 1)), ('b', (c - 1,)), ('dy', (0, 5, h - 1, w - 2))):
                for kind in KINDS:
                    out.append(Case('ban', (shape, act), '%s %s' % ('x'.join(map(str, shape)), act), ban_make(shape), (inp, idx, kind), ban_oracle,
                                    ban_unreachable, 2e-5, path='bias_act_noise fwd+bwd', may_vanish=(act == 'relu' and inp != 'dy' and kind != '+inf')))
    return out


# ----------------------------------------------------------------------------- upfirdn_2d
# (name, major, H, W, C, kshape, up, down, pad0, pad1, path, zero_extended)
UPFIRDN = [
    ('fir4 4x4 taps', 2, 17, 17, 8, 4, 1, 1, 1, 1, 'fir4 fast path', False),
    ('fir4 3x3 taps', 1, 5, 7, 4, 3, 1, 1, 1, 1, 'fir4 fast path, zero-extended', True),
    ('fir4 1x1 taps', 1, 7, 7, 4, 1, 1, 1, 0, 0, 'fir4 fast path, zero-extended', True),
    ('generic up 2', 2, 8, 8, 3, 4, 2, 1, 2, 1, 'generic', False),
    ('generic down 2', 2, 16, 16, 3, 4, 1, 2, 1, 2, 'generic', False),
    ('generic C%4', 3, 9, 6, 5, 4, 1, 1, 0, 3, 'generic', False),
]


def upfirdn_kw(cfg):
    _name, _m, _h, _w, _c, _ks, up, down, p0, p1 = cfg[:10]
    return dict(upx=up, upy=up, downx=down, downy=down, padx0=p0, padx1=p1, pady0=p0, pady1=p1)


def upfirdn_out_hw(cfg):
    _name, _m, h, w, _c, ks, up, down, p0, p1 = cfg[:10]
    return (h * up + p0 + p1 - ks + down) // down, (w * up + p0 + p1 - ks + down) // down


def upfirdn_make(cfg):
    def make():
        _name, m, h, w, c, ks = cfg[:6]
        rng = np.random.RandomState(m * 1000 + h * 10 + ks)
        oh, ow = upfirdn_out_hw(cfg)
        return dict(x=rng.randn(m, h, w, c), dy=rng.randn(m, oh, ow, c), k=rng.rand(ks, ks) + 0.1)
    return make


def upfirdn_oracle(cfg, t):
    from oracle import upfirdn_2d as O
    x = t['x'].clone().requires_grad_(True)
    y = O.upfirdn_2d_ref(x, t['k'].numpy(), **upfirdn_kw(cfg))
    (dx,) = torch.autograd.grad(y, x, t['dy'])
    return dict(y=y.detach(), dx=dx)


def upfirdn_unreachable(cfg, poison, shapes):
    """Depth-wise per sample: every other (sample, channel) plane; the output that the poisoned input does not feed is out of reach as a whole."""
    inp, idx, _ = poison
    name, other = ('y', 'dx') if inp == 'x' else ('dx', 'y')
    m = np.ones(shapes[name], dtype=bool)
    m[idx[0], :, :, idx[3]] = False
    return {name: m, other: _all(shapes[other])}


def upfirdn_reach(cfg, poison, shapes):
    """The 4x4 footprint of the zero-extended fast path (forward: pad0; gradient: the flipped filter with pad k - pad0 - 1)."""
    inp, idx, _ = poison
    ks, p0 = cfg[5], cfg[8]
    name, pad = ('y', p0) if inp == 'x' else ('dx', ks - p0 - 1)
    m = np.zeros(shapes[name], dtype=bool)
    hh, ww = shapes[name][1], shapes[name][2]
    m[idx[0], max(idx[1] + pad - 3, 0):min(idx[1] + pad, hh - 1) + 1, max(idx[2] + pad - 3, 0):min(idx[2] + pad, ww - 1) + 1, idx[3]] = True
    return {name: m}


def upfirdn_cases():
    out = []
    for cfg in UPFIRDN:
        name, m, h, w, c = cfg[:5]
        oh, ow = upfirdn_out_hw(cfg)
        for inp, idx in (('x', (m - 1, h // 2, w // 2 + 1, c - 2)), ('dy', (0, oh // 2 + 1, ow // 2, 1))):
            for kind in KINDS:
                out.append(Case('upfirdn', cfg, name, upfirdn_make(cfg), (inp, idx, kind), upfirdn_oracle, upfirdn_unreachable, 2e-6,
                                reach=upfirdn_reach if cfg[11] else None, exact_mask=not cfg[11], path=cfg[10]))
    return out


# FirBanFn: the FIR after an up-convolution + noise + bias + lrelu in one pass, on the first shape (logical NCHW)
FIRBAN = ('fir4 4x4 + lrelu', 2, 17, 17, 8, 4, 1, 1, 1, 1, 'fir4 fast path + epilogue', False)


def firban_make():
    d = upfirdn_make(FIRBAN)()
    rng = np.random.RandomState(77)
    oh, ow = upfirdn_out_hw(FIRBAN)
    d.update(b=rng.randn(FIRBAN[4]), noise=rng.randn(FIRBAN[1], 1, oh, ow))
    return d


def firban_oracle(cfg, t):
    """Inputs in the FIR's [major, H, W, C] layout; results likewise (the op itself takes logical NCHW)."""
    from oracle import upfirdn_2d as O
    idx, alpha, gain = BAN_ACTS['lrelu']
    x = t['x'].clone().requires_grad_(True)
    f = O.upfirdn_2d_ref(x, t['k'].numpy(), **upfirdn_kw(cfg))
    nz = t['noise'].permute(0, 2, 3, 1)
    y = _kernel_ref(f + nz * BAN_STRENGTH + t['b'].view(1, 1, 1, -1), None, 0, idx, alpha, gain)
    dpre = _kernel_ref(t['dy'], y.detach(), 1, idx, alpha, gain)
    (dx,) = torch.autograd.grad(f, x, dpre)
    return dict(y=y.detach(), dx=dx, db=dpre.sum(dim=(0, 1, 2)), ds=(dpre * nz).sum())


def firban_unreachable(cfg, poison, shapes):
    inp, idx, _ = poison
    un = upfirdn_unreachable(cfg, poison, shapes)
    if inp == 'x':      # the select of the gradient form reads y: the poisoned (sample, channel) plane of dx is within reach of a poisoned x as well
        un['dx'] = np.ones(shapes['dx'], dtype=bool)
        un['dx'][idx[0], :, :, idx[3]] = False
    un['db'] = _other(shapes['db'], 0, idx[3])
    return un


def firban_cases():
    return [Case('firban', FIRBAN, FIRBAN[0], firban_make, (inp, idx, kind), firban_oracle, firban_unreachable, 2e-5, path=FIRBAN[10])
            for inp, idx in (('x', (1, 8, 9, 6)), ('dy', (0, 9, 8, 1))) for kind in KINDS]


# ----------------------------------------------------------------------------- conv2d forward / data gradient / weight gradient
def conv_oracle_fn(x, w, pad, out_hw):
    """The _conv_oracle formulation of tests/test_gpu_ops.py at stride 1 without up-sampling: pad, correlate, crop (fp64)."""
    kh, kw = w.shape[0], w.shape[1]
    oh, ow = out_hw
    pad_b = max(oh - 1 + kh - pad - x.shape[2], 0)
    pad_r = max(ow - 1 + kw - pad - x.shape[3], 0)
    y = F.conv2d(F.pad(x, [pad, pad_r, pad, pad_b]), w.permute(3, 2, 0, 1))
    return y[:, :, :oh, :ow]


# (name, N, Cin, H, W, Cout, K, path)
CONVS = [
    ('2x16x9x7->40 3x3', 2, 16, 9, 7, 40, 3, 'fp32 MFMA tile'),
    ('3x512x4x4->512 3x3', 3, 512, 4, 4, 512, 3, 'split-K 4x4 layer'),
    ('3x128x9x7->3 1x1', 3, 128, 9, 7, 3, 1, 'thin output'),
    ('2x3x12x12->64 3x3', 2, 3, 12, 12, 64, 3, 'thin input'),
    ('7x64x1x1->40 1x1', 7, 64, 1, 1, 40, 1, 'small dense'),
]
CONV_PIECE = ('1x128x32x32->128 3x3', 1, 128, 32, 32, 128, 3, 'fp16 piece form')
CONV_ALPHA = 0.73


def conv_make(cfg):
    def make():
        _name, n, cin, h, w, cout, k = cfg[:7]
        rng = np.random.RandomState(n * 131 + cin + cout)
        return dict(x=rng.randn(n, cin, h, w), w=rng.randn(k, k, cin, cout) / np.sqrt(k * k * cin), dy=rng.randn(n, cout, h, w), s=rng.rand(n, cin) + 0.5)
    return make


def conv_oracle(cfg, t):
    """y = conv(x * s, w) * alpha; dx = its gradient w.r.t. the scaled input, dw w.r.t. the filter (what conv2d_raw / conv2d_wgrad_raw return)."""
    k = cfg[6]
    xs = (t['x'] * t['s'][:, :, None, None]).requires_grad_(True)
    w = t['w'].clone().requires_grad_(True)
    y = conv_oracle_fn(xs, w, k // 2, (cfg[3], cfg[4])) * CONV_ALPHA
    dx, dw = torch.autograd.grad(y, [xs, w], t['dy'])
    return dict(y=y.detach(), dx=dx, dw=dw)


def _window_miss(shape, n, h, w, k):
    """True for every element of an [N, C, H, W] tensor outside sample n's k x k window around (h, w)."""
    m = np.ones(shape, dtype=bool)
    r = k // 2
    m[n, :, max(h - r, 0):h + r + 1, max(w - r, 0):w + r + 1] = False
    return m


def conv_unreachable(cfg, poison, shapes):
    inp, idx, _ = poison
    k = cfg[6]
    if inp == 'x':       # other samples and the output pixels whose window misses the poisoned pixel; the data gradient never reads x
        return dict(y=_window_miss(shapes['y'], idx[0], idx[2], idx[3], k), dx=_all(shapes['dx']), dw=_other(shapes['dw'], 2, idx[1]))
    if inp == 's':
        return dict(y=_other(shapes['y'], 0, idx[0]), dx=_all(shapes['dx']), dw=_other(shapes['dw'], 2, idx[1]))
    if inp == 'w':       # [kh, kw, c, o]: output channel o of y, input channel c of dx; the weight gradient never reads w
        return dict(y=_other(shapes['y'], 1, idx[3]), dx=_other(shapes['dx'], 1, idx[2]), dw=_all(shapes['dw']))
    return dict(y=_all(shapes['y']), dx=_window_miss(shapes['dx'], idx[0], idx[2], idx[3], k), dw=_other(shapes['dw'], 3, idx[1]))      # dy


def conv_mask_only(cfg, inp):
    """Outputs the poison reaches by more than a quarter by construction (module docstring)."""
    _name, n, cin, h, w, cout, k = cfg[:7]
    out = []
    if inp == 's' and n < 4:
        out.append('y')                 # a whole sample of a batch of 1..3
    if inp == 'w' and cout < 4:
        out.append('y')                 # one of three output channels
    if inp == 'w' and cin < 4:
        out.append('dx')
    if inp in ('x', 's') and cin < 4:
        out.append('dw')                # one of three input channels
    if inp == 'dy' and cout < 4:
        out.append('dw')
    return out


def conv_poisons(cfg):
    """Interior pixel (every tap of the weight gradient meets it) and the centre tap (no output pixel sees it through the padding only)."""
    _name, n, cin, h, w, cout, k = cfg[:7]
    ph, pw = (h // 2, w // 2 - (1 if w > 2 else 0)) if h > 1 else (0, 0)
    return (('x', (n - 1, cin - 2, ph, pw)), ('w', (k // 2, k // 2, 1, cout - 2)), ('dy', (0, cout - 1, ph, pw)), ('s', (n - 1, 2)))


def conv_cases(piece=False):
    out = []
    for cfg in ([CONV_PIECE] if piece else CONVS):
        for inp, idx in conv_poisons(cfg):
            for kind in KINDS:
                out.append(Case('conv', cfg, cfg[0], conv_make(cfg), (inp, idx, kind), conv_oracle, conv_unreachable, 3e-5,
                                mask_only=conv_mask_only(cfg, inp), path=cfg[7]))
    return out


# ModConv2dFn (scales folded into the kernel) and ConvBiasActFn (lrelu in the epilogue), one shape each
MODCONV = ('modconv 3x20x6x6->28 3x3', 3, 20, 6, 6, 28, 3, 'ModConv2dFn')
CBA = ('conv+bias+lrelu 2x16x9x9->24 3x3', 2, 16, 9, 9, 24, 3, 'ConvBiasActFn', 'lrelu')
CBA_RELU = ('conv+bias+relu 2x16x9x9->24 3x3', 2, 16, 9, 9, 24, 3, 'ConvBiasActFn (the LPIPS VGG epilogue)', 'relu')
CBA_ALPHA = 0.8


def modconv_make():
    d = conv_make(MODCONV)()
    d['d'] = np.random.RandomState(12).rand(MODCONV[1], MODCONV[5]) + 0.5
    return d


def modconv_oracle(cfg, t):
    ins = [t[k].clone().requires_grad_(True) for k in ('x', 'w', 's', 'd')]
    x, w, s, d = ins
    y = conv_oracle_fn(x * s[:, :, None, None], w, 1, (cfg[3], cfg[4])) * d[:, :, None, None]
    dx, dw, ds, dd = torch.autograd.grad(y, ins, t['dy'])
    return dict(y=y.detach(), dx=dx, dw=dw, ds=ds, dd=dd)


def modconv_unreachable(cfg, poison, shapes):
    inp, idx, _ = poison
    n = idx[0]
    if inp == 's':      # (n, c): sample n of y, dd; plane (n, c) of dx; input channel c of dw; ds does not read s
        dx = np.ones(shapes['dx'], dtype=bool)
        dx[idx[0], idx[1]] = False
        return dict(y=_other(shapes['y'], 0, n), dx=dx, dw=_other(shapes['dw'], 2, idx[1]), ds=_all(shapes['ds']), dd=_other(shapes['dd'], 0, n))
    if inp == 'w':      # [kh, kw, c, o]: output channel o of y and dd, input channel c of dx and ds; dw does not read w
        return dict(y=_other(shapes['y'], 1, idx[3]), dx=_other(shapes['dx'], 1, idx[2]), dw=_all(shapes['dw']), ds=_other(shapes['ds'], 1, idx[2]),
                    dd=_other(shapes['dd'], 1, idx[3]))
    if inp == 'x':
        return dict(y=_window_miss(shapes['y'], n, idx[2], idx[3], 3), dx=_all(shapes['dx']), dw=_other(shapes['dw'], 2, idx[1]),
                    ds=_other(shapes['ds'], 0, n), dd=_other(shapes['dd'], 0, n))
    return dict(y=_all(shapes['y']), dx=_window_miss(shapes['dx'], n, idx[2], idx[3], 3), dw=_other(shapes['dw'], 3, idx[1]),
                ds=_other(shapes['ds'], 0, n), dd=_other(shapes['dd'], 0, n))


def cba_make():
    d = conv_make(CBA)()
    d['b'] = np.random.RandomState(13).randn(CBA[5]) * 0.3
    d['b'][11] = 4.0                   # keeps unit (0, 11, 5, 4), where dy is poisoned, active under relu as well (checked from the oracle side)
    del d['s']
    return d


def cba_oracle(cfg, t):
    idx, alpha, gain = BAN_ACTS[cfg[8]]
    x = t['x'].clone().requires_grad_(True)
    w = t['w'].clone().requires_grad_(True)
    pre = conv_oracle_fn(x, w, 1, (cfg[3], cfg[4])) * CBA_ALPHA
    y = _kernel_ref(pre.detach() + t['b'].view(1, -1, 1, 1), None, 0, idx, alpha, gain)
    dpre = _kernel_ref(t['dy'], y, 1, idx, alpha, gain)
    dx, dw = torch.autograd.grad(pre, [x, w], dpre)
    return dict(y=y, dx=dx, dw=dw, db=dpre.sum(dim=(0, 2, 3)))


def cba_unreachable(cfg, poison, shapes):
    inp, idx, _ = poison
    n = idx[0]
    if inp == 'x':      # the select of the gradient form sees the poisoned window: within sample n only other samples' dx are out of reach
        # and every channel of dw and db sums over the window whose select changed
        return dict(y=_window_miss(shapes['y'], n, idx[2], idx[3], 3), dx=_other(shapes['dx'], 0, n))
    return dict(y=_all(shapes['y']), dx=_window_miss(shapes['dx'], n, idx[2], idx[3], 3), dw=_other(shapes['dw'], 3, idx[1]), db=_other(shapes['db'], 0, idx[1]))


def fused_conv_cases():
    out = []
    for kind in KINDS:
        out.append(Case('modconv', MODCONV, MODCONV[0], modconv_make, ('x', (2, 7, 3, 2), kind), modconv_oracle, modconv_unreachable,
                        dict(y=3e-5, dx=5e-5, dw=5e-5, ds=5e-5, dd=5e-5), mask_only=('dd',), path=MODCONV[7]))
        out.append(Case('modconv', MODCONV, MODCONV[0], modconv_make, ('dy', (0, 20, 2, 3), kind), modconv_oracle, modconv_unreachable,
                        dict(y=3e-5, dx=5e-5, dw=5e-5, ds=5e-5, dd=5e-5), mask_only=('ds',), path=MODCONV[7]))
        for cfg in (CBA, CBA_RELU):
            out.append(Case('cba', cfg, cfg[0], cba_make, ('x', (1, 9, 4, 5), kind), cba_oracle, cba_unreachable, 3e-5, path=cfg[7]))
            out.append(Case('cba', cfg, cfg[0], cba_make, ('dy', (0, 11, 5, 4), kind), cba_oracle, cba_unreachable, 3e-5, path=cfg[7]))
        for inp, idx, mo in (('s', (2, 7), ('y', 'dd')), ('w', (1, 1, 7, 20), ())):
            out.append(Case('modconv', MODCONV, MODCONV[0], modconv_make, (inp, idx, kind), modconv_oracle, modconv_unreachable,
                            dict(y=3e-5, dx=5e-5, dw=5e-5, ds=5e-5, dd=5e-5), mask_only=mo, path=MODCONV[7]))
    return out


# ----------------------------------------------------------------------------- style path (s, d)
STYLES = [(6, 512, 128, 3, 1, False), (32, 64, 36, 20, 3, True)]


def style_make(cfg):
    def make():
        n, l, cin, cout, k, _demod = cfg
        rng = np.random.RandomState(n + cin)
        return dict(y=rng.randn(n, l), A=rng.randn(l, cin), b=rng.randn(cin) * 0.1, w=rng.randn(k, k, cin, cout))
    return make


def style_oracle(cfg, t):
    n, l, cin, cout, k, demod = cfg
    c_a, c_w = 1.0 / np.sqrt(l), 1.0 / np.sqrt(k * k * cin)
    s = c_a * (t['y'] @ t['A']) + t['b'] + 1.0
    out = dict(s=s)
    if demod:
        out['d'] = torch.rsqrt(c_w * c_w * ((s * s) @ (t['w'] * t['w']).sum(dim=(0, 1))) + 1e-8)
    return out


def style_unreachable(cfg, poison, shapes):
    inp, idx, _ = poison
    un = {}
    if inp == 'y':
        un = {k: _other(v, 0, idx[0]) for k, v in shapes.items()}
    elif inp == 'A':
        un = dict(s=_other(shapes['s'], 1, idx[1]))          # every d sums over the poisoned channel
    else:
        un = dict(s=_all(shapes['s']))
        if 'd' in shapes:
            un['d'] = _other(shapes['d'], 1, idx[3])
    return un


def style_cases():
    out = []
    for cfg in STYLES:
        n, l, cin, cout, k, demod = cfg
        poisons = [('y', (n - 2, l - 3)), ('A', (5, cin - 1))] + ([('w', (k - 1, 0, 3, cout - 2))] if demod else [])     # without demodulation w is not read
        for inp, idx in poisons:
            for kind in KINDS:
                out.append(Case('style', cfg, 'N%d L%d %d->%d k%d%s' % (n, l, cin, cout, k, ' demod' if demod else ''), style_make(cfg), (inp, idx, kind),
                                style_oracle, style_unreachable, 1e-5, mask_only=('d',) if (inp == 'A' and demod and kind == 'nan') else (), path='style_mod',
                                may_vanish=(inp == 'w' and kind != 'nan')))      # s = +-inf or w = +-inf: d = rsqrt(inf) = 0, finite by IEEE arithmetic on both sides
    return out


# ----------------------------------------------------------------------------- minibatch stddev
MBSTD = [((8, 16, 4, 4), 4), ((4, 64, 4, 4), 2)]       # the second: 64 * 16 = 1024 positions, the statistic is summed over four slices


def mbstd_make(cfg):
    def make():
        shape, g = cfg
        rng = np.random.RandomState(shape[0] * 10 + g)
        return dict(x=rng.randn(*shape), dy=rng.randn(shape[0], shape[1] + 1, shape[2], shape[3]))
    return make


def mbstd_oracle(cfg, t):
    from oracle import networks_stylegan2 as ON
    x = t['x'].clone().requires_grad_(True)
    y = ON.minibatch_stddev_layer(x, cfg[1])
    (dx,) = torch.autograd.grad(y, x, t['dy'])
    return dict(y=y.detach(), dx=dx)


def mbstd_unreachable(cfg, poison, shapes):
    """Sample n shares its statistic with the samples n' = n (mod M), M = N / G: the other residues' statistic channel and gradients, and every
    pass-through element but the poisoned one, are out of reach."""
    (n_all, c, _h, _w), g = cfg
    m_ = n_all // min(g, n_all)
    inp, idx, _ = poison
    same = np.array([(i % m_) == (idx[0] % m_) for i in range(n_all)])
    y = np.ones(shapes['y'], dtype=bool)
    dx = np.ones(shapes['dx'], dtype=bool)
    if inp == 'x':
        y[same, c] = False
        y[idx] = False
        dx[same, idx[1], idx[2], idx[3]] = False       # the statistic's gradient at a position reads that position of the group only
    else:
        if idx[1] == c:
            dx[same] = False                           # the statistic channel's cotangent reaches every element of the group
        else:
            dx[idx] = False
    return dict(y=y, dx=dx)


def mbstd_cases():
    out = []
    for cfg in MBSTD:
        (n, c, h, w), g = cfg
        for inp, idx in (('x', (n - 3, c - 5, 2, 1)), ('dy', (1, 3, 0, 2)), ('dy', (n - 1, c, 3, 3))):
            for kind in KINDS:
                out.append(Case('mbstd', cfg, '%s G%d' % ('x'.join(map(str, cfg[0])), g), mbstd_make(cfg), (inp, idx, kind), mbstd_oracle, mbstd_unreachable,
                                1e-5, mask_only=('dx',) if (inp == 'dy' and idx[1] == c) else (), path='mbstd fwd+bwd'))
    return out


# ----------------------------------------------------------------------------- LPIPS layer distance
LPIPS_SHAPE = (3, 64, 16, 16)


def lpips_make():
    n, c, h, w = LPIPS_SHAPE
    rng = np.random.RandomState(c + h)
    return dict(fa=np.maximum(rng.randn(n, c, h, w), 0.0) + 0.01, fb=np.maximum(rng.randn(n, c, h, w) + 0.3, 0.0) + 0.01, lin=np.abs(rng.randn(c)) / c, g=rng.randn(n))


def lpips_oracle(cfg, t):
    """oracle/lpips.py:31,38 as tests/test_gpu_ops.py test_lpips_layer_distance states it."""
    a = t['fa'].clone().requires_grad_(True)
    b = t['fb'].clone().requires_grad_(True)
    ua = a / (torch.sqrt(torch.sum(a * a, dim=1, keepdim=True)) + 1e-10)
    ub = b / (torch.sqrt(torch.sum(b * b, dim=1, keepdim=True)) + 1e-10)
    d = ((ua - ub) ** 2 * t['lin'].view(1, -1, 1, 1)).sum(dim=(1, 2, 3))
    ga, gb = torch.autograd.grad(d, [a, b], t['g'])
    return dict(d=d.detach(), ga=ga, gb=gb)


def lpips_unreachable(cfg, poison, shapes):
    n = poison[1][0]
    return dict(d=_other(shapes['d'], 0, n), ga=_other(shapes['ga'], 0, n), gb=_other(shapes['gb'], 0, n))


def lpips_cases():
    return [Case('lpips', LPIPS_SHAPE, 'x'.join(map(str, LPIPS_SHAPE)), lpips_make, ('fa', (0, 17, 5, 9), kind), lpips_oracle, lpips_unreachable,
                 dict(d=1e-5, ga=2e-5, gb=2e-5), mask_only=('d',), path='LpipsLayerFn') for kind in KINDS]


def all_cases():
    return ban_cases() + upfirdn_cases() + firban_cases() + conv_cases() + conv_cases(piece=True) + fused_conv_cases() + style_cases() + mbstd_cases() + lpips_cases()


# ----------------------------------------------------------------------------- fused_bias_act: the special-value vector
FBA_SPECIALS = [np.nan, np.inf, -np.inf, 100.0, -100.0, 81.0, -81.0, 79.0, -79.0, 41.0, -41.0, 39.0, -39.0, 0.0, -0.0, FLT_MAX, 1e-30]


def fba_vectors(n):
    """x and ref of n elements: the special values against each other (ref is x rotated by 7 within the specials, so that every special meets
    several partners over the sizes used) followed by randn."""
    rng = np.random.RandomState(n)
    k = len(FBA_SPECIALS)
    assert n > k
    sp = np.array(FBA_SPECIALS, dtype=np.float32)
    x = np.concatenate([sp, rng.randn(n - k)]).astype(np.float32)
    ref = np.concatenate([np.roll(sp, 7), rng.randn(n - k) * 0.7]).astype(np.float32)
    return x, ref


def fba_oracle(x, b, ref, grad, act_idx, alpha, gain, step_b):
    """(values in fp64, non-finite set): the set is that of the restated formulas evaluated in the kernel's own format, fp32 -- 1 - ref * ref at
    ref = FLT_MAX is -inf there and a large finite number in fp64 --, the values are the fp64 evaluation."""
    from oracle.fused_bias_act import fused_bias_act_kernel_ref
    t = lambda a, dt: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dt)
    y64 = fused_bias_act_kernel_ref(t(x, torch.float64), t(b, torch.float64), t(ref, torch.float64), grad, act_idx, alpha, gain, step_b)
    y32 = fused_bias_act_kernel_ref(t(x, torch.float32), t(b, torch.float32), t(ref, torch.float32), grad, act_idx, np.float32(alpha).item(), np.float32(gain).item(), step_b)
    return y64, ~torch.isfinite(y32)


# ----------------------------------------------------------------------------- finite check / Adam
ADAM_TWO_PASS = 2048 * 256 * 4 + 4099        # one whole grid of float4s (2048 blocks x 256 lanes) + 1024 float4s of a second pass + 3 scalar tail elements
ADAM_SIZES = [1, 3, 4, 5, 1023, 10007, ADAM_TWO_PASS]
FINITE_SPECIALS = [FLT_MAX, -FLT_MAX, float(np.float32(1.4e-45)), -0.0]


def adam_positions(n):
    """Index 0, n - 1 (in the scalar tail when n % 4 != 0), the last element of the vector body, and -- where there is one -- an index of the second
    grid-stride pass."""
    pos = {0, n - 1}
    if n >= 4:
        pos.add((n // 4) * 4 - 1)
    if n > 2048 * 256 * 4:
        pos.add(2048 * 256 * 4 + 2049)
    return sorted(pos)


# ----------------------------------------------------------------------------- max-pool windows
def pool_input():
    """[1, 64, 8, 8] post-ReLU features with, in channel 3, 2x2 windows holding: one NaN; two NaNs; NaN next to +inf; -inf only (with finite others)."""
    rng = np.random.RandomState(64)
    x = np.maximum(rng.randn(1, 64, 8, 8), 0).astype(np.float32)
    c = 3
    x[0, c, 0, 1] = np.nan                                   # window (0, 0): one NaN
    x[0, c, 0, 2] = np.nan; x[0, c, 1, 3] = np.nan           # window (0, 1): two NaNs
    x[0, c, 2, 0] = np.inf; x[0, c, 2, 1] = np.nan           # window (1, 0): NaN after +inf
    x[0, c, 3, 2] = np.nan; x[0, c, 3, 3] = np.inf           # window (1, 1): NaN before +inf
    x[0, c, 4, 4] = -np.inf                                  # window (2, 2): one -inf among finite values
    x[0, c, 6:8, 6:8] = -np.inf                              # window (3, 3): -inf only
    return x, rng.randn(1, 64, 8, 8).astype(np.float32), rng.randn(1, 64, 4, 4).astype(np.float32)
