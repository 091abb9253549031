"""The thin-channel convolution kernels (csrc/thin_conv.hip) restated in fp64 from include/igan_hip.h -- the comment blocks of
igan_conv2d_params and igan_conv2d_wgrad_params -- with the case tables, the input generator and an fp32 model of the kernels' summation
shared by tests/test_thin_cases.py (host) and tests/test_gpu_thin_conv.py.  NumPy only: no device is needed to import it.  The arena,
the sentinel and the input helpers are those of tests/dense_cases.py.

Inputs are fp32 values; every reference widens them to double first.  A tensor is seeded by its name, its form and its shape; values
lean positive (randn + 0.5), so that no output is a cancelled sum.  "Loud" (positive, magnitude in [1, 2)) are the last channel quad of
the wide operand (of x and of the filter), the last pixel of the tensor, the last pixel of every workgroup's pixel range in the weight
gradient and, under a 3x3 filter, the border rows and columns of x: a kernel that loses exactly that moves an output by a known share.

Two bounds, both per case (the GPU test holds both; the host test holds the inputs to them with the fp32 model and the mutants):
  (a) tests.util.rel_err < 3e-5 against the restatement -- the bar tests/test_gpu_ops.py holds these kernels to;
  (b) per element |got - ref| <= 1.01 (T + 4) 2^-24 S, T the element's number of in-range terms and S its fp64 sum of absolute terms:
      any order of fp32 additions of T products stays within (T - 1) roundings of S, the in_scale, alpha and out_scale multiplications add
      at most four.  Derived, not measured.  For a weight gradient T = N HW makes (b) loose: (a) governs there, (b) is only printed.

Which kernel takes a shape (thin_conv_kind / thin_conv / thin_wgrad_kind; every row below states the name the library must report):
  thin_out_kernel<taps>   stride = up = 1, act = 0, 1x1 (pad 0, OH = H, OW = W) or 3x3, 16-byte aligned operands, Cout <= 4, Cin / 4 a power
                          of two, 64 <= Cin <= 512 (1x1) or 256 (3x3).  <1> covers one and two channel blocks (Cin = 512).
  thin_in_kernel<taps>    the same, Cin <= 4, Cout / 4 a power of two, 16 <= Cout <= 512, no in_scale.  <9> ALSO stands for the sliding-window
                          kernel thin_in3x3_kernel<3>, which takes a 3x3 shape when  Cin == 3  and  Cout <= 256  and  OW >= 16  (the name
                          does not tell the two apart: FWD_IN and FWD_SLIDE keep cases on both sides of each of the three conditions, and
                          whichever kernel takes a shape is held to the same reference).
  thin_wgrad_kernel       1x1, stride = up = 1, pad 0, same size, aligned operands; Cout <= 4 without out_scale or Cin <= 4 without in_scale, the
                          wide side C a multiple of 4 in [16, 1024] with 256 % (C / 4) == 0.  At the launch a missing, short or misaligned
                          workspace sends the call to the tile kernels (the reported name is the plan's and stays).
A 1x1 call on a 1x1 map without scales is a small dense layer (dense_small.hip) before it is a thin one: the one-pixel cases carry a scale."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from dense_cases import GUARD, SENTINEL, Arena, _fma32, _lean, _loud, _rng, rel_err64      # noqa: F401 -- re-exported for the two test files

ALPHA = float(np.float32(0.7))
GAIN = float(np.float32(1.5))       # act = 1 (linear) without a bias: y * gain
BOUND_A = 3e-5
EPS24 = 2.0 ** -24


def bound_b(S, T):
    return 1.01 * (np.asarray(T, np.float64) + 4.0) * EPS24 * S


def ratio_b(got, ref, S, T):
    """max over the elements of |got - ref| / bound (b); an element without terms must be exactly zero."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    b = np.broadcast_to(bound_b(S, T), err.shape)
    r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


# ----------------------------------------------------------------------------- fp64 restatement
def filter64(w, wt, KH, KW, Cin, Cout, flip=True, swap=True):
    """W(ky, kx, ci, co) of the header: w[ky][kx][ci][co], or w[KH-1-ky][KW-1-kx][co][ci] when w_transposed.  flip / swap off: the mutants."""
    w = np.asarray(w, np.float64)
    if not wt:
        return w.reshape(KH, KW, Cin, Cout)
    w = w.reshape(KH, KW, Cout, Cin)
    if flip:
        w = w[::-1, ::-1]
    return w.transpose(0, 1, 3, 2) if swap else np.ascontiguousarray(w).reshape(KH, KW, Cin, Cout)


def _taps(H, W, OH, OW, KH, KW, pad_y, pad_x, stride=1, up=1, clamp=False, cols=None):
    """One entry per tap: (ky, kx, iy [OH], ix [OW], in-range mask [OH, OW]) with xup[v] = x[v / up] where v % up == 0 and in range.
    clamp: out-of-range reads take the nearest pixel instead of zero (a mutant); cols(kx, ox, ix, ok) -> (ix, ok) rewrites a tap's columns."""
    oy, ox = np.arange(OH), np.arange(OW)
    for ky in range(KH):
        vy = oy * stride + ky - pad_y
        iy, oky = vy // up, (vy >= 0) & (vy % up == 0) & (vy // up < H)
        for kx in range(KW):
            vx = ox * stride + kx - pad_x
            ix, okx = vx // up, (vx >= 0) & (vx % up == 0) & (vx // up < W)
            if cols is not None:
                ix, okx = cols(kx, ox, ix, okx)
            if clamp:
                oky, okx = np.ones(OH, bool), np.ones(OW, bool)
            yield ky, kx, np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1), oky[:, None] & okx[None, :]


def conv(x, w, *, KH, KW, Cout, wt=False, in_scale=None, out_scale=None, alpha=1.0, pad_y=0, pad_x=0, OH=None, OW=None, stride=1, up=1, gain=1.0,
         flip=True, swap=True, clamp=False, cols=None):
    """y[n, oy, ox, co] = gain alpha out_scale[n, co] sum_{ky, kx, ci} xup[n, oy stride + ky - pad_y, ox stride + kx - pad_x, ci] in_scale[n, ci] W(ky, kx, ci, co),
    a direct loop over the taps.  -> (y, S, T): S the sum of the absolute terms of each element, T [1, OH, OW, 1] its number of in-range terms."""
    x = np.asarray(x, np.float64)
    N, H, W_, Cin = x.shape
    Wf = filter64(w, wt, KH, KW, Cin, Cout, flip, swap)
    if in_scale is not None:
        x = x * np.asarray(in_scale, np.float64)[:, None, None, :]
    y, S, T = np.zeros((N, OH, OW, Cout)), np.zeros((N, OH, OW, Cout)), np.zeros((OH, OW), np.int64)
    for ky, kx, iy, ix, ok in _taps(H, W_, OH, OW, KH, KW, pad_y, pad_x, stride, up, clamp, cols):
        g = x[:, iy][:, :, ix] * ok[None, :, :, None]
        y += g @ Wf[ky, kx]
        S += np.abs(g) @ np.abs(Wf[ky, kx])
        T += ok * Cin
    f = np.full((1, 1, 1, 1), alpha * gain) if out_scale is None else alpha * gain * np.asarray(out_scale, np.float64)[:, None, None, :]
    return y * f, S * np.abs(f), T[None, :, :, None]


def wgrad(x, dy, *, KH, KW, in_scale=None, out_scale=None, alpha=1.0, pad_y=0, pad_x=0, stride=1, up=1, keep=None):
    """dw[ky, kx, ci, co] = alpha sum_{n, oy, ox} xup[n, oy stride + ky - pad_y, ox stride + kx - pad_x, ci] in_scale[n, ci] dy[n, oy, ox, co] out_scale[n, co],
    in chunks of samples.  keep [N, OH, OW] (optional): the output pixels a mutant still sums.  -> (dw, S, T [KH, KW, 1, 1])."""
    N, H, W_, Cin = x.shape
    _, OH, OW, Cout = dy.shape
    dw, S, T = np.zeros((KH, KW, Cin, Cout)), np.zeros((KH, KW, Cin, Cout)), np.zeros((KH, KW, 1, 1), np.int64)
    step = max(1, (1 << 21) // max(1, H * W_ * Cin, OH * OW * Cout))
    for n0 in range(0, N, step):
        n1 = min(N, n0 + step)
        xs, d = np.asarray(x[n0:n1], np.float64), np.asarray(dy[n0:n1], np.float64)
        if in_scale is not None:
            xs = xs * np.asarray(in_scale[n0:n1], np.float64)[:, None, None, :]
        if out_scale is not None:
            d = d * np.asarray(out_scale[n0:n1], np.float64)[:, None, None, :]
        if keep is not None:
            d = d * keep[n0:n1, :, :, None]
        d2, a2 = d.reshape(-1, Cout), np.abs(d).reshape(-1, Cout)
        for ky, kx, iy, ix, ok in _taps(H, W_, OH, OW, KH, KW, pad_y, pad_x, stride, up):
            g = (xs[:, iy][:, :, ix] * ok[None, :, :, None]).reshape(-1, Cin)
            dw[ky, kx] += g.T @ d2
            S[ky, kx] += np.abs(g).T @ a2
            T[ky, kx] += int(ok.sum()) * (n1 - n0)
    return alpha * dw, abs(alpha) * S, T


# ----------------------------------------------------------------------------- case tables
# A forward (or data-gradient) call.  pad < 0: SAME ((k - 1) / 2); OH, OW = 0: H + 2 pad - (k - 1).  xoff: floats between the arena's
# 16-byte boundary and x.
Fwd = namedtuple('Fwd', 'name N H W Cin Cout k pad_y pad_x OH OW wt isc osc stride up act xoff')


def F(name, N, H, W, Cin, Cout, k=1, pad=-1, OH=0, OW=0, wt=0, isc=0, osc=0, stride=1, up=1, act=0, xoff=0):
    pad_y, pad_x = pad if isinstance(pad, tuple) else (pad, pad)
    pad_y, pad_x = ((k - 1) // 2 if pad_y < 0 else pad_y), ((k - 1) // 2 if pad_x < 0 else pad_x)
    return Fwd(name, N, H, W, Cin, Cout, k, pad_y, pad_x, OH or H + 2 * pad_y - (k - 1), OW or W + 2 * pad_x - (k - 1), wt, isc, osc, stride, up, act, xoff)


OUT1, OUT9, IN1, IN9 = 'thin_out_kernel<1>', 'thin_out_kernel<9>', 'thin_in_kernel<1>', 'thin_in_kernel<9>'
NOT_THIN_FWD, NOT_THIN_WGRAD = 'conv_fwd_', 'conv_wgrad_kernel'      # the families a shape outside thin_*_kind runs on (the forward name goes on with the tile)
SCALES = ((0, 0), (1, 0), (0, 1), (1, 1))


def _out_1x1():
    """thin_out_kernel<1>: a group of gw = min(Cin / 4, 64) lanes per pixel, 64 / gw pixels per wave and step, four steps in flight: a wave's trip
    takes 16 (Cin 64), 8 (Cin 128) or 4 (Cin 256, 512) pixels.  Per Cin: one pixel (with a scale: see the module text), one pixel less and
    one more than a trip, and the largest one-workgroup count that is one less than a whole trip: every wave makes two trips, the second of the
    last wave is ragged.  Cout, the filter layout and the four scale combinations cycle over the rows of a Cin (each Cout meets every one)."""
    rows = []
    shapes = {64: [(1, 1, 1), (1, 3, 5), (1, 1, 17), (1, 127, 1)],      # 16 lanes per pixel: 1, 15, 17, 127 pixels
              128: [(1, 1, 1), (1, 7, 1), (3, 1, 3), (3, 3, 7)],        # 32 lanes per pixel: 1, 7, 9, 63
              256: [(1, 1, 1), (3, 1, 1), (1, 5, 1), (1, 1, 31)],       # 64 lanes per pixel: 1, 3, 5, 31
              512: [(1, 1, 1), (1, 3, 1), (5, 1, 1), (1, 31, 1)]}       # 64 lanes per pixel, two channel blocks (thin_out_kernel<1, 2>)
    i = 0
    for Cin, shp in shapes.items():
        for N, H, W in shp:
            for Cout in (1, 2, 3, 4):
                isc, osc = SCALES[(i + i // 4 + Cout) % 4]
                if H == 1 and W == 1 and not (isc or osc):
                    isc = 1
                rows.append(F(OUT1, N, H, W, Cin, Cout, wt=(i // 4 + Cout) % 2, isc=isc, osc=osc))
            i += 1
    rows += [F(OUT1, 3, 2, 3, 64, 3, wt=w, isc=s[0], osc=s[1]) for w in (0, 1) for s in SCALES]      # ToRGB's Cout under every scale combination, three samples
    return rows


def _out_3x3():
    """thin_out_kernel<9>: one pixel step per trip (4 pixels per wave at Cin 64, 1 at Cin 256)."""
    rows = []
    for i, Cin in enumerate((64, 256)):
        for j, (H, W, pad, OH, OW) in enumerate([(9, 7, 1, 0, 0),               # SAME: 63 pixels per sample, two trips per wave
                                                  (5, 4, 0, 0, 0),               # VALID: OH = H - 2 (what the data gradient of a pad-2 layer asks for)
                                                  (2, 3, 2, 0, 0),               # pad 2, OH = H + 2: the data gradient of a VALID convolution
                                                  (4, 3, (0, 2), 0, 0),          # pad_y != pad_x: OH = H - 2, OW = W + 2
                                                  (1, 1, 1, 0, 0)]):             # a single pixel: one tap in range
            for Cout in (1, 2, 3, 4):
                isc, osc = SCALES[(i + j + Cout) % 4]
                rows.append(F(OUT9, 2, H, W, Cin, Cout, 3, pad, OH, OW, wt=(j + Cout) % 2, isc=isc, osc=osc))
    return rows


def _in_1x1():
    """thin_in_kernel<1>: cg = min(Cout / 4, 64) lanes per pixel, 64 / cg pixels per wave and trip: 16 (Cout 16), 4 (Cout 64), 1 (Cout 256, and 512 in two
    channel blocks).  Per Cout: one pixel (with out_scale), one less and one more than a trip, and a count that gives every wave two trips."""
    rows = []
    shapes = {16: [(1, 1, 1), (1, 3, 5), (1, 17, 1), (1, 1, 127)],      # 1, 15, 17, 127
              64: [(1, 1, 1), (3, 1, 1), (1, 1, 5), (1, 31, 1)],        # 1, 3, 5, 31
              256: [(1, 1, 1), (1, 2, 1), (3, 3, 1)],                   # 1, 2, 9
              512: [(1, 1, 1), (2, 1, 1), (3, 1, 3)]}                   # 1, 2, 9: the second channel block
    i = 0
    for Cout, shp in shapes.items():
        for N, H, W in shp:
            for Cin in (1, 2, 3, 4):
                osc = (i + Cin) % 2 or int(H == 1 and W == 1)
                rows.append(F(IN1, N, H, W, Cin, Cout, wt=(i // 2 + Cin) % 2, osc=osc))
            i += 1
    return rows


def _in_3x3():
    """thin_in_kernel<9>, the generic kernel: every 3x3 thin-input shape that fails one of the sliding kernel's three conditions."""
    rows = []
    for j, (H, W, pad) in enumerate([(9, 7, 1), (5, 4, 0), (2, 3, 2), (4, 3, (0, 2)), (1, 1, 1), (3, 18, 1)]):      # the geometries of _out_3x3, and OW = 18
        for i, (Cin, Cout) in enumerate([(1, 16), (4, 64), (2, 256), (1, 512), (4, 16)]):                            # Cin != 3: never the sliding kernel
            rows.append(F(IN9, 2, H, W, Cin, Cout, 3, pad, wt=(i + j) % 2, osc=(i + j // 2) % 2))
    for wt in (0, 1):
        rows += [F(IN9, 2, 3, 16, 3, 512, 3, wt=wt, osc=wt),            # Cin 3, OW 16, Cout 512: two channel blocks, not the sliding kernel
                 F(IN9, 2, 3, 15, 3, 64, 3, wt=wt, osc=1 - wt),         # Cin 3, Cout 64, OW 15: one column short of it
                 F(IN9, 2, 3, 17, 3, 256, 3, 0, wt=wt, osc=wt),         # pad 0: W 17 gives OW 15
                 F(IN9, 2, 3, 16, 4, 64, 3, wt=wt, osc=1 - wt),         # Cin 4 at OW 16
                 F(IN9, 1, 1, 12, 3, 64, 3, wt=wt)]                     # VGG conv1_1 at a small width
    return rows


def _slide():
    """thin_in3x3_kernel<3> (reported as thin_in_kernel<9>): Cin 3, Cout <= 256, OW >= 16.  A lane walks a run of 32 output pixels three at a time:
    OW 16 / 17 / 32 / 33 / 34 / 35 / 65 give runs of 16 | 17 | 32 | 32 + 1 | 32 + 2 | 32 + 3 | 32 + 32 + 1 pixels, i.e. run tails (length % 3) of
    1, 2, 2, 1, 2, 0 and runs that start at x = 32 and x = 64.  H 1, 2: every input row is a border row; H 5: some are.  pad 0, 1, 2 with OW following
    (W = OW + 2 - 2 pad; pad 0 needs H >= 3)."""
    rows, i = [], 0
    for OW in (16, 17, 32, 33, 34, 35, 65):
        for H, pad in ((1, 1), (1, 2), (2, 1), (2, 2), (5, 0), (5, 1), (5, 2)):
            rows.append(F(IN9, (1, 3)[i % 2], H, OW + 2 - 2 * pad, 3, (16, 64, 256)[i % 3], 3, pad, wt=(i // 2) % 2, osc=(i // 3) % 2))
            i += 1
    return rows


FWD_OUT1, FWD_OUT9, FWD_IN1, FWD_IN9, FWD_SLIDE = _out_1x1(), _out_3x3(), _in_1x1(), _in_3x3(), _slide()

# Shapes that must LEAVE the family and still be right: each pins one condition of thin_conv_kind.
FWD_LEAVE = [
    F(NOT_THIN_FWD, 2, 3, 5, 32, 3, isc=1),                    # Cin 32: 8 lanes per pixel would break the 16-value reduce-scatter of thin_out
    F(NOT_THIN_FWD, 2, 3, 5, 48, 3),                           # Cin 48: 12 lanes, not a power of two
    F(NOT_THIN_FWD, 2, 3, 5, 512, 3, 3),                       # Cin 512 at 3x3: two channel blocks of nine taps do not fit the registers
    F(NOT_THIN_FWD, 2, 3, 5, 64, 5, osc=1),                    # Cout 5
    F(NOT_THIN_FWD, 2, 9, 7, 64, 3, 3, 0, 4, 3, stride=2),     # stride 2 (VALID, as the discriminator's down-sampling convolution)
    F(NOT_THIN_FWD, 2, 4, 5, 64, 3, 3, 2, 9, 11, wt=1, up=2),  # up 2 (the transposed convolution of the generator's up-sampling layers)
    F(NOT_THIN_FWD, 2, 3, 5, 64, 3, 1, 1),                     # 1x1 with pad 1: OH = H + 2
    F(NOT_THIN_FWD, 2, 3, 5, 3, 64, isc=1),                    # in_scale on a thin-input call
    F(NOT_THIN_FWD, 2, 3, 5, 64, 3, act=1),                    # a fused epilogue (linear, no bias, gain 1.5)
    F(NOT_THIN_FWD, 2, 3, 5, 64, 3, xoff=1),                   # x 4 bytes past a 16-byte boundary
    F(NOT_THIN_FWD, 2, 3, 5, 3, 64, 3, xoff=1),                # the same in front of a 3x3 thin-input shape
]

# A weight-gradient call: orientation 'out' (Cout = T <= 4, wide x [N, HW, C], optional in_scale) or 'in' (Cin = T, wide dy, optional out_scale).
# ws: 'plan' | 'null' | 'short' (one float less than the plan) | 'offset' (the plan's size, 4 bytes past a 16-byte boundary).
Wg = namedtuple('Wg', 'name orient N H W C T k isc osc ws')


def G(name, orient, N, H, W, C, T, scale=0, k=1, isc=None, osc=None, ws='plan'):
    """scale: the wide side's scale (in_scale of a thin-output call, out_scale of a thin-input call), the only one the thin kernel takes."""
    isc = (scale if orient == 'out' else 0) if isc is None else isc
    osc = (scale if orient == 'in' else 0) if osc is None else osc
    return Wg(name, orient, N, H, W, C, T, k, isc, osc, ws)


WGRAD = 'thin_wgrad_kernel'


def wgrad_bps(N, HW):
    """Workgroups per sample (thin_wgrad_bps): enough to fill the machine, at least 64 pixels each."""
    return max(1, min(-(-1536 // N), HW // 64 if HW >= 64 else 1))


def wgrad_block_ends(N, HW):
    """The last pixel of every workgroup's range within a sample."""
    bps = wgrad_bps(N, HW)
    per = -(-HW // bps)
    return [min((b + 1) * per, HW) - 1 for b in range(bps) if b * per < HW]


def _wgrad_rows():
    """thin_wgrad_kernel: C / 4 = 4, 16, 64, 256 lanes per pixel (64 ... 1 pixel sub-lanes per workgroup).  (N, H, W): HW = 1 at N = 24 (one pixel per workgroup;
    without a scale and with T = 4 on the wide side's other end this is a small dense layer, see the module text, so these rows carry a scale or the thin output);
    HW = 63: one workgroup per sample; HW = 129, 200 at N = 3: two workgroups of 65 + 64 and three of 67 + 67 + 66 pixels."""
    rows, i = [], 0
    for C in (16, 64, 256, 1024):
        for N, H, W in ((24, 1, 1), (2, 9, 7), (3, 3, 43), (3, 8, 25)):
            for orient in ('out', 'in'):
                for T in (1, 2, 3, 4):
                    scale = (i + T) % 2
                    if H * W == 1 and (orient == 'in' or T == 4):
                        scale = 1
                    rows.append(G(WGRAD, orient, N, H, W, C, T, scale))
                i += 1
    return rows


WGRAD_ROWS = _wgrad_rows()
# the second 1024-pixel slab of a workgroup (the LDS refill behind its barrier): one workgroup per sample, 1025 pixels, the loud last pixel alone in the second slab
WGRAD_SLAB = [G(WGRAD, 'out', 1536, 25, 41, 16, 3, 1)]
# the launch-time fallbacks: the plan says thin, the workspace the caller passes cannot serve it, the tile kernels run (N bps >= 3, so that the short
# workspace still holds the two partial filters of the tile kernels' split)
WGRAD_FALLBACK = [G(WGRAD, 'out', 3, 3, 43, 64, 3, 1, ws='null'), G(WGRAD, 'in', 3, 3, 43, 64, 3, 1, ws='null'),
                  G(WGRAD, 'out', 3, 3, 43, 64, 3, 1, ws='short'), G(WGRAD, 'in', 3, 8, 25, 16, 4, 0, ws='short'),
                  G(WGRAD, 'out', 3, 3, 43, 64, 3, 1, ws='offset'), G(WGRAD, 'in', 3, 8, 25, 16, 4, 0, ws='offset')]
WGRAD_LEAVE = [
    G(NOT_THIN_WGRAD, 'out', 2, 9, 7, 64, 3, isc=1, osc=1),      # out_scale on a thin-output call
    G(NOT_THIN_WGRAD, 'in', 2, 9, 7, 64, 3, isc=1, osc=1),       # in_scale on a thin-input call
    G(NOT_THIN_WGRAD, 'out', 2, 9, 7, 20, 3, 1),                 # C = 20: five lanes per pixel do not divide a workgroup
    G(NOT_THIN_WGRAD, 'out', 2, 9, 7, 64, 3, 1, k=3),            # a 3x3 filter
]


# ----------------------------------------------------------------------------- inputs
def _scales(name, key, N, C):
    """Per-sample scales, distinct, in [0.5, 1.5)."""
    s = _rng(name, *key).uniform(0.5, 1.5, size=(N, C)).astype(np.float32)
    assert len({tuple(r) for r in s}) == N
    return s


@functools.lru_cache(maxsize=None)
def fwd_case(r):
    """One forward problem: fp32 operands as the kernel reads them (w in its stored layout), and ref = (y, S, T).  Cached and shared: never written to."""
    key = tuple(r)[1:]
    taps = r.k * r.k
    x = _lean(_rng('x', *key), (r.N, r.H, r.W, r.Cin))
    W = _rng('w', *key).standard_normal((r.k, r.k, r.Cin, r.Cout)) + 0.5
    if r.Cin > 4:       # thin output: the last channel quad of x and of the filter
        x[..., -4:] = _loud(x[..., -4:])
        W[:, :, -4:, :] = _loud(W[:, :, -4:, :])
    else:               # thin input: the last quad of output channels
        W[..., -4:] = _loud(W[..., -4:])
    x[-1, -1, -1] = _loud(x[-1, -1, -1])
    if taps > 1:
        for edge in (x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1]):
            edge[...] = _loud(edge)
    K = taps * r.Cin
    W = (W / (0.25 * K + np.sqrt(K))).astype(np.float32)
    c = SimpleNamespace(r=r, x=x, W=W, w=np.ascontiguousarray(W[::-1, ::-1].transpose(0, 1, 3, 2)) if r.wt else W,
                        in_scale=_scales('isc', key, r.N, r.Cin) if r.isc else None, out_scale=_scales('osc', key, r.N, r.Cout) if r.osc else None,
                        alpha=ALPHA, gain=GAIN if r.act else 1.0)
    c.ref = fwd_of(c)
    for a in (c.x, c.W, c.w, c.in_scale, c.out_scale) + c.ref:
        if a is not None:
            a.setflags(write=False)
    return c


def fwd_of(c, **over):
    """conv() on a case's operands; `over` replaces arguments (the mutants)."""
    r = c.r
    kw = dict(x=c.x, w=c.w, KH=r.k, KW=r.k, Cout=r.Cout, wt=bool(r.wt), in_scale=c.in_scale, out_scale=c.out_scale, alpha=c.alpha, pad_y=r.pad_y, pad_x=r.pad_x,
              OH=r.OH, OW=r.OW, stride=r.stride, up=r.up, gain=c.gain)
    kw.update(over)
    return conv(kw.pop('x'), kw.pop('w'), **kw)


@functools.lru_cache(maxsize=None)
def wgrad_case(r):
    """One weight-gradient problem.  x [N, H, W, Cin], dy [N, OH, OW, Cout] (OH = H, OW = W: pad (k - 1) / 2), ref = (dw [k, k, Cin, Cout], S, T)."""
    key = tuple(r)[1:-1]
    Cin, Cout = (r.C, r.T) if r.orient == 'out' else (r.T, r.C)
    x = _lean(_rng('wg.x', *key), (r.N, r.H, r.W, Cin))
    dy = _lean(_rng('wg.dy', *key), (r.N, r.H, r.W, Cout))
    wide = x if r.orient == 'out' else dy
    wide[..., -4:] = _loud(wide[..., -4:])
    for t in (x, dy):
        f = t.reshape(r.N, r.H * r.W, -1)
        for e in wgrad_block_ends(r.N, r.H * r.W):
            f[:, e] = _loud(f[:, e])
    c = SimpleNamespace(r=r, x=x, dy=dy, Cin=Cin, Cout=Cout, in_scale=_scales('wg.isc', key, r.N, Cin) if r.isc else None,
                        out_scale=_scales('wg.osc', key, r.N, Cout) if r.osc else None, alpha=ALPHA, pad=(r.k - 1) // 2)
    c.ref = wgrad_of(c)
    for a in (c.x, c.dy, c.in_scale, c.out_scale) + c.ref:
        if a is not None:
            a.setflags(write=False)
    return c


def wgrad_of(c, keep=None, **over):
    kw = dict(KH=c.r.k, KW=c.r.k, in_scale=c.in_scale, out_scale=c.out_scale, alpha=c.alpha, pad_y=c.pad, pad_x=c.pad, keep=keep)
    kw.update(over)
    return wgrad(c.x, c.dy, **kw)


def wgrad_plan_floats(r):
    """The workspace igan_conv2d_wgrad_plan() must ask for on a thin row (thin_wgrad_workspace)."""
    return max(r.N * wgrad_bps(r.N, r.H * r.W) * r.C * 4, 2 * r.C * r.T)


# ----------------------------------------------------------------------------- fp32 model of the kernels' summation
def _gather32(x, r):
    """x as each tap reads it, zero where out of range: [(ky, kx, [N, OH, OW, Cin] fp32)]."""
    return [(ky, kx, (x[:, iy][:, :, ix] * ok[None, :, :, None]).astype(np.float32))
            for ky, kx, iy, ix, ok in _taps(r.H, r.W, r.OH, r.OW, r.k, r.k, r.pad_y, r.pad_x, r.stride, r.up)]


def fwd_model32(c):
    """The arithmetic of thin_out / thin_in in fp32.  Thin output: x * in_scale rounded, lane l of a pixel's gw sums its channel quads over the channel blocks and
    taps with four fused multiply-adds per quad (innermost the quad's last element), the lanes are added as a butterfly (1, 2, 4, ...), then alpha, then out_scale.
    Thin input: one fused multiply-add per tap and channel in order, then alpha, then out_scale.  Shapes outside the family are modelled as thin input (a plain
    fused multiply-add chain over taps and channels).  -> y [N, OH, OW, Cout] fp32."""
    r, f = c.r, np.float32
    q = c.x if c.in_scale is None else c.x * c.in_scale[:, None, None, :]
    taps = _gather32(q, r)
    if r.Cout <= 4 and r.Cin >= 64 and r.Cin % 4 == 0 and (r.Cin // 4) & (r.Cin // 4 - 1) == 0:
        gw = min(r.Cin // 4, 64)
        acc = np.zeros((gw, r.N, r.OH, r.OW, r.Cout), f)
        for cb in range(r.Cin // (4 * gw)):
            for ky, kx, g in taps:
                for e in (3, 2, 1, 0):
                    ci = 4 * (np.arange(gw) + gw * cb) + e
                    acc = _fma32(np.moveaxis(g[..., ci], -1, 0)[..., None], c.W[ky, kx, ci][:, None, None, None, :], acc)
        while acc.shape[0] > 1:
            acc = acc[0::2] + acc[1::2]
        acc = acc[0]
    else:
        acc = np.zeros((r.N, r.OH, r.OW, r.Cout), f)
        for ky, kx, g in taps:
            for ci in range(r.Cin):
                acc = _fma32(g[..., ci, None], c.W[ky, kx, ci][None, None, None, :], acc)
    y = acc * f(c.alpha)
    if c.out_scale is not None:
        y = y * c.out_scale[:, None, None, :]
    return y * f(c.gain) if r.act else y


def wgrad_model32(c):
    """thin_wgrad in fp32: within a workgroup pixel p goes to sub-lane (p - p0) % (256 / cg), which adds its pixels in order with one fused multiply-add each; the
    sub-lanes are added in order, the scale multiplies the workgroup's partial; lane l of the final wave adds the workgroups l, l + 64, ... in order, the 64 lanes
    are added as a tree, alpha last.  1x1 rows only.  -> dw [1, 1, Cin, Cout] fp32."""
    r, f = c.r, np.float32
    HW = r.H * r.W
    wide = (c.x if r.orient == 'out' else c.dy).reshape(r.N, HW, r.C)
    thin = (c.dy if r.orient == 'out' else c.x).reshape(r.N, HW, r.T)
    scale = c.in_scale if r.orient == 'out' else c.out_scale
    ppb = 256 // min(r.C // 4, 256)
    bps = wgrad_bps(r.N, HW)
    per = -(-HW // bps)
    parts = []
    for b in range(bps):
        p0, p1 = b * per, min((b + 1) * per, HW)
        acc = np.zeros((r.N, ppb, r.C, r.T), f)
        for s in range(p0, p1, ppb):
            idx = s + np.arange(ppb)
            ok = (idx < p1)[None, :, None]
            idx = np.minimum(idx, p1 - 1)
            acc = _fma32((wide[:, idx] * ok)[..., None], (thin[:, idx] * ok)[:, :, None, :], acc)
        part = np.zeros((r.N, r.C, r.T), f)
        for q in range(ppb):
            part = part + acc[:, q]
        parts.append(part if scale is None else part * scale[:, :, None])
    blocks = np.stack(parts, axis=1).reshape(r.N * bps, r.C, r.T)      # workgroup index n * bps + b
    lanes = np.zeros((64, r.C, r.T), f)
    for b0 in range(0, blocks.shape[0], 64):
        chunk = blocks[b0:b0 + 64]
        lanes[:chunk.shape[0]] = lanes[:chunk.shape[0]] + chunk
    while lanes.shape[0] > 1:
        lanes = lanes[0::2] + lanes[1::2]
    dw = lanes[0] * f(c.alpha)
    return (dw if r.orient == 'out' else dw.T).reshape(1, 1, c.Cin, c.Cout)


# ----------------------------------------------------------------------------- arena placement and struct fields
def place_fwd(arena, c, workspace_floats=0):
    r = c.r
    arena.put('x', np.concatenate([np.full(r.xoff, SENTINEL, np.float32), c.x.ravel()]))
    arena.put('w', c.w)
    if c.in_scale is not None:
        arena.put('in_scale', c.in_scale)
    if c.out_scale is not None:
        arena.put('out_scale', c.out_scale)
    arena.reserve('y', (r.N, r.OH, r.OW, r.Cout))
    if workspace_floats:
        arena.reserve('workspace', (workspace_floats,))


def fwd_fields(r, addr, plan=(1, 0, 0)):
    """Fields of igan_conv2d_params; addr(name, extra floats) -> device address or None; plan = (splits, sliced_tiles, workspace_floats) of igan_conv2d_plan()."""
    return dict(x=addr('x', r.xoff), w=addr('w', 0), y=addr('y', 0), in_scale=addr('in_scale', 0) if r.isc else None, out_scale=addr('out_scale', 0) if r.osc else None,
                workspace=addr('workspace', 0) if plan[2] else None, workspace_floats=plan[2], N=r.N, H=r.H, W=r.W, Cin=r.Cin, OH=r.OH, OW=r.OW, Cout=r.Cout,
                KH=r.k, KW=r.k, stride=r.stride, up=r.up, pad_y=r.pad_y, pad_x=r.pad_x, w_transposed=r.wt, splits=plan[0], sliced_tiles=plan[1], alpha=ALPHA,
                bias=None, act=r.act, act_alpha=0.0, act_gain=GAIN if r.act else 1.0)


def place_wgrad(arena, c, plan_floats):
    """The workspace region has the plan's size ('plan', and 'short': the call is told one float less), four floats more for 'offset', none for 'null'."""
    r = c.r
    arena.put('x', c.x)
    arena.put('dy', c.dy)
    if c.in_scale is not None:
        arena.put('in_scale', c.in_scale)
    if c.out_scale is not None:
        arena.put('out_scale', c.out_scale)
    arena.reserve('dw', (r.k, r.k, c.Cin, c.Cout))
    if r.ws != 'null' and plan_floats:
        arena.reserve('workspace', (plan_floats + (4 if r.ws == 'offset' else 0),))


def wgrad_fields(c, addr, plan):
    """Fields of igan_conv2d_wgrad_params; plan = (splits, workspace_floats) of igan_conv2d_wgrad_plan().  A call without a workspace cannot split: splits = 1."""
    r = c.r
    has_ws = r.ws != 'null' and plan[1] > 0
    return dict(x=addr('x', 0), dy=addr('dy', 0), dw=addr('dw', 0), in_scale=addr('in_scale', 0) if r.isc else None, out_scale=addr('out_scale', 0) if r.osc else None,
                workspace=addr('workspace', 1 if r.ws == 'offset' else 0) if has_ws else None, workspace_floats=(plan[1] - (1 if r.ws == 'short' else 0)) if has_ws else 0,
                N=r.N, H=r.H, W=r.W, Cin=c.Cin, OH=r.H, OW=r.W, Cout=c.Cout, KH=r.k, KW=r.k, stride=1, up=1, pad_y=c.pad, pad_x=c.pad,
                splits=plan[0] if has_ws else 1, alpha=ALPHA)
