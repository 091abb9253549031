"""GPU: a NaN or an infinity goes through every training op the way the fp64 oracle says -- never laundered into a finite number, never spread
to results that have nothing to do with it.  Optimizer.apply_updates() protects the weights by ONE finite check over the flat gradient bucket
(csrc/optimizer.hip); that check is worth what the kernels between a poisoned activation and the bucket carry through (DESIGN.md "Non-finite values").

Cases, oracles and the four shared assertions (no laundering / bit-identical isolation / values to the existing tolerances / extra non-finite
elements only inside a declared reach) are in tests/nonfinite_cases.py; tests/test_nonfinite_cases.py checks the cases from the oracle side.

Where the contract is the reference kernel's select and NOT the framework's function (the oracle there is the restated select,
oracle.fused_bias_act.fused_bias_act_kernel_ref, not torch.relu):
    relu(NaN) = 0 and relu(-inf) = 0 (x > 0 ? x : 0), lrelu(NaN) = NaN, and the gradient forms select on ref = y / gain the same way --
    fused_bias_act_raw, bias_act_noise, the FIR epilogue (FirBanFn) and the convolution epilogue (ConvBiasActFn).
Declared reaches of extra non-finite elements (HIP non-finite where the oracle is finite):
    * upfirdn_2d fast path with fewer than 4x4 taps (3x3, 1x1): the taps are zero-extended to 4x4 and 0 * inf = NaN, so an input reaches the 4x4
      footprint oy in [iy + pad0 - 3, iy + pad0], ox likewise, same sample and channel (the gradient: the same with pad k - pad0 - 1).  The 4x4
      filter on the fast path and every generic-path case must match the oracle's set exactly.
    * the fp16 piece form of the convolutions: the poisoned element's scale group (a pixel's channels for the forward / data-gradient image,
      a channel's pixels for the weight gradient's, an output channel's taps for the filter's).  The cases put the poison at an interior pixel /
      the centre tap, where the oracle's own set is the whole group, so no extra element is expected; what a border pixel does to the weight
      gradient is printed (profiles/nonfinite.txt), not asserted.
Every case prints a NONFINITE line (op, path, poison, oracle / HIP / extra counts): profiles/nonfinite.txt is that output on the MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import nonfinite_cases as NC
from tests.util import rel_err, to_nhwc_cuda

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


# ----------------------------------------------------------------------------- HIP side of every case family: inputs (NumPy fp32) -> results
def run_ban(case, t, device):
    from inclusivegan_amd import hip_ops
    _shape, act = case.cfg
    idx, alpha, gain = NC.BAN_ACTS[act]
    x = to_nhwc_cuda(torch.from_numpy(t['x']), device).requires_grad_(True)
    b = _dev(t['b'], device).requires_grad_(True)
    st = torch.tensor(NC.BAN_STRENGTH, device=device, requires_grad=True)
    y = hip_ops.bias_act_noise(x, b, _dev(t['noise'], device), st, idx, alpha, gain)
    dx, db, ds = torch.autograd.grad(y, [x, b, st], to_nhwc_cuda(torch.from_numpy(t['dy']), device))
    return dict(y=y, dx=dx, db=db, ds=ds)


def run_upfirdn(case, t, device):
    from inclusivegan_amd.dnnlib.tflib.ops.upfirdn_2d import upfirdn_2d
    x = _dev(t['x'], device).requires_grad_(True)
    y = upfirdn_2d(x, t['k'], **NC.upfirdn_kw(case.cfg))
    (dx,) = torch.autograd.grad(y, x, _dev(t['dy'], device))
    return dict(y=y, dx=dx)


def run_firban(case, t, device):
    from inclusivegan_amd import hip_ops
    idx, alpha, gain = NC.BAN_ACTS['lrelu']
    nchw = lambda a: _dev(a, device).permute(0, 3, 1, 2)          # [N, H, W, C] dense = logical NCHW with channels_last strides
    x = nchw(t['x']).requires_grad_(True)
    b = _dev(t['b'], device).requires_grad_(True)
    st = torch.tensor(NC.BAN_STRENGTH, device=device, requires_grad=True)
    y = hip_ops.FirBanFn.apply(x, t['k'], case.cfg[8], case.cfg[9], b, _dev(t['noise'], device), st, idx, alpha, gain)
    dx, db, ds = torch.autograd.grad(y, [x, b, st], nchw(t['dy']))
    return dict(y=y.permute(0, 2, 3, 1), dx=dx.permute(0, 2, 3, 1), db=db, ds=ds)


def run_conv(case, t, device):
    from inclusivegan_amd import hip_ops
    _name, n, cin, h, w, cout, k = case.cfg[:7]
    geom = hip_ops.ConvGeom(k, k, 1, 1, k // 2, k // 2, NC.CONV_ALPHA)
    x = to_nhwc_cuda(torch.from_numpy(t['x']), device)
    dy = to_nhwc_cuda(torch.from_numpy(t['dy']), device)
    wt, s = _dev(t['w'], device), _dev(t['s'], device)
    y = hip_ops.conv2d_raw(x, wt, geom, (h, w), cout, in_scale=s)
    dx = hip_ops.conv2d_raw(dy, wt, hip_ops.dgrad_geom(geom), (h, w), cin, w_transposed=True)
    dw = hip_ops.conv2d_wgrad_raw(x, dy, geom, in_scale=s)
    return dict(y=y, dx=dx, dw=dw)


def run_modconv(case, t, device):
    from inclusivegan_amd import hip_ops
    _name, n, cin, h, w, cout, k = case.cfg[:7]
    ins = [to_nhwc_cuda(torch.from_numpy(t['x']), device).requires_grad_(True)] + [_dev(t[q], device).requires_grad_(True) for q in ('w', 's', 'd')]
    y = hip_ops.ModConv2dFn.apply(*ins, hip_ops.ConvGeom(k, k, 1, 1, 1, 1), (h, w))
    dx, dw, ds, dd = torch.autograd.grad(y, ins, to_nhwc_cuda(torch.from_numpy(t['dy']), device))
    return dict(y=y, dx=dx, dw=dw, ds=ds, dd=dd)


def run_cba(case, t, device):
    from inclusivegan_amd import hip_ops
    _name, n, cin, h, w, cout, k = case.cfg[:7]
    idx, alpha, gain = NC.BAN_ACTS[case.cfg[8]]
    ins = [to_nhwc_cuda(torch.from_numpy(t['x']), device).requires_grad_(True)] + [_dev(t[q], device).requires_grad_(True) for q in ('w', 'b')]
    assert hip_ops.conv_bias_act_fusable(ins[0], cout, idx)
    y = hip_ops.ConvBiasActFn.apply(*ins, hip_ops.ConvGeom(k, k, 1, 1, 1, 1, NC.CBA_ALPHA), (h, w), idx, alpha, gain)
    dx, dw, db = torch.autograd.grad(y, ins, to_nhwc_cuda(torch.from_numpy(t['dy']), device))
    return dict(y=y, dx=dx, dw=dw, db=db)


def run_style(case, t, device):
    from inclusivegan_amd import hip_ops
    n, l, cin, cout, k, demod = case.cfg
    yfull = torch.zeros(n, 3, l, device=device)
    yfull[:, 1] = _dev(t['y'], device)                              # a strided [N, L] slice like dlatents[:, i]
    a, b, w = (_dev(t[q], device) for q in ('A', 'b', 'w'))
    wsq = hip_ops.sumsq_taps_raw(w) if demod else None
    assert hip_ops.style_mod_fusable(yfull[:, 1], a, w, demod)
    s, d = hip_ops.style_mod(yfull.unbind(1)[1], a, b, w, wsq, 1.0 / np.sqrt(l), 1.0 / np.sqrt(k * k * cin), demod)
    return dict(s=s, d=d) if demod else dict(s=s)


def run_mbstd(case, t, device):
    from inclusivegan_amd.training.networks_stylegan2 import minibatch_stddev_layer
    x = to_nhwc_cuda(torch.from_numpy(t['x']), device).requires_grad_(True)
    y = minibatch_stddev_layer(x, case.cfg[1])
    (dx,) = torch.autograd.grad(y, x, to_nhwc_cuda(torch.from_numpy(t['dy']), device))
    return dict(y=y, dx=dx)


def run_lpips(case, t, device):
    from inclusivegan_amd import hip_ops
    a = to_nhwc_cuda(torch.from_numpy(t['fa']), device).requires_grad_(True)
    b = to_nhwc_cuda(torch.from_numpy(t['fb']), device).requires_grad_(True)
    d = hip_ops.LpipsLayerFn.apply(a, b, _dev(t['lin'], device))
    ga, gb = torch.autograd.grad(d, [a, b], _dev(t['g'], device))
    return dict(d=d, ga=ga, gb=gb)


RUNNERS = dict(ban=run_ban, upfirdn=run_upfirdn, firban=run_firban, conv=run_conv, modconv=run_modconv, cba=run_cba, style=run_style,
               mbstd=run_mbstd, lpips=run_lpips)
_clean = {}


def run_case(case, device):
    """HIP on the clean input (once per op and shape: the isolation check compares against it bit for bit) and on the poisoned one, fp64 oracle on the
    poisoned one, then the four assertions."""
    key = (case.op, case.cfg)
    if key not in _clean:
        _clean[key] = {k: v.detach().cpu().contiguous() for k, v in RUNNERS[case.op](case, case.inputs(False), device).items()}
    got = {k: v.detach().cpu().contiguous() for k, v in RUNNERS[case.op](case, case.inputs(True), device).items()}
    return NC.check_outputs(case, case.want(), got, _clean[key])


CASES = [c for c in NC.all_cases() if c.cfg is not NC.CONV_PIECE]


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_nonfinite_case(case, cuda_device):
    """One poisoned element through one op: the four assertions of tests/nonfinite_cases.py (module docstring there and here)."""
    if case.op == 'conv':       # below the piece form's thresholds (3x3 on >= 128 channels over >= 1024 rows): the same kernels under every form
        assert case.cfg[2] < 128 or case.cfg[6] == 1 or case.cfg[1] * case.cfg[3] * case.cfg[4] < 1024
    run_case(case, cuda_device)


# ----------------------------------------------------------------------------- the default piece form, in a child process with the form stated
PIECE_CHILD = r'''
import ctypes, sys
import torch
sys.path.insert(0, %r)
from inclusivegan_amd import hip_ops, _abi
from tests import nonfinite_cases as NC
from tests import test_gpu_nonfinite as T
dev = torch.device('cuda', 0)
lib = _abi.get_plugin()
assert lib.igan_conv_piece_form() == 2
_name, n, cin, h, w, cout, k = NC.CONV_PIECE[:7]
buf = ctypes.create_string_buffer(128)
for transposed, (ci, co) in ((0, (cin, cout)), (1, (cout, cin))):
    p = _abi.Conv2DParams(x=1 << 20, w=1 << 20, y=1 << 20, in_scale=(None if transposed else 1 << 20), out_scale=None, workspace=None, workspace_floats=0, N=n, H=h, W=w, Cin=ci,
                          OH=h, OW=w, Cout=co, KH=k, KW=k, stride=1, up=1, pad_y=k // 2, pad_x=k // 2, w_transposed=transposed, splits=1, alpha=NC.CONV_ALPHA, bias=None, act=0,
                          act_alpha=0.0, act_gain=1.0)
    _abi.check(lib.igan_conv2d_kernel_name(ctypes.byref(p), buf, 128))
    assert buf.value.decode().startswith('conv_fwd_planes'), buf.value.decode()
    print('KERNEL ' + ('dgrad ' if transposed else 'fwd ') + buf.value.decode())
pw = _abi.Conv2DWgradParams(x=1 << 20, dy=1 << 20, dw=1 << 20, in_scale=1 << 20, out_scale=None, workspace=None, workspace_floats=0, N=n, H=h, W=w, Cin=cin, OH=h, OW=w, Cout=cout,
                            KH=k, KW=k, stride=1, up=1, pad_y=k // 2, pad_x=k // 2, splits=1, alpha=NC.CONV_ALPHA)
_abi.check(lib.igan_conv2d_wgrad_kernel_name(ctypes.byref(pw), buf, 128))
assert buf.value.decode() == 'conv_wgrad_planes_kernel', buf.value.decode()
print('KERNEL wgrad ' + buf.value.decode())
for case in NC.conv_cases(piece=True):
    T.run_case(case, dev)
# observation, not an assertion: a BORDER pixel.  Some taps of the poisoned channel miss it and stay finite in the oracle, while the column image's
# per-channel scale has seen it
base = [c for c in NC.conv_cases(piece=True) if c.poison[0] == 'x']
for case in base:
    inp, idx, kind = case.poison
    case.poison = (inp, (idx[0], idx[1], 0, 0), kind)
    t = case.inputs(True)
    got = T.run_conv(case, t, dev)['dw'].cpu()
    want = case.want()['dw']
    o_bad, h_bad = NC.nonfinite32(want), ~torch.isfinite(got)
    ch = idx[1]
    fin = ~o_bad[:, :, ch, :] & ~h_bad[:, :, ch, :]
    err = float((got.double()[:, :, ch, :][fin] - want[:, :, ch, :][fin]).abs().max() / want[:, :, ch, :][~o_bad[:, :, ch, :]].abs().max()) if bool(fin.any()) else float('nan')
    other = torch.ones_like(o_bad); other[:, :, ch, :] = False
    print('NONFINITE-BORDER conv wgrad %%s fp16 piece form  poison %%-5s at x[%%d,%%d,0,0]  dw channel %%d: oracle non-finite %%d of %%d, hip non-finite %%d, finite in both %%d (rel err there %%.2e); other channels: hip non-finite %%d'
          %% (NC.CONV_PIECE[0], kind, idx[0], ch, ch, int(o_bad[:, :, ch, :].sum()), o_bad[:, :, ch, :].numel(), int(h_bad[:, :, ch, :].sum()), int(fin.sum()), err, int(h_bad[other].sum())))
print('NONFINITE-PIECE-OK')
'''


def test_nonfinite_piece_form(cuda_device):
    """The twelve convolution cases at (1,128,32,32 -> 128, 3x3), the smallest shape that takes the default fp16 piece form in all three kernels
    (asserted with igan_conv2d_kernel_name / igan_conv2d_wgrad_kernel_name), in a child process with IGAN_CONV_PLANES=2 and the row thresholds stated."""
    env = dict(os.environ, IGAN_CONV_PLANES='2', IGAN_PLANES_MIN_ROWS='1024', IGAN_WGRAD_PLANES_MIN_ROWS='1024')
    r = subprocess.run([sys.executable, '-c', PIECE_CHILD % ROOT], env=env, capture_output=True, text=True, timeout=600)
    sys.stdout.write(''.join(ln + '\n' for ln in r.stdout.splitlines() if ln.startswith(('NONFINITE', 'KERNEL'))))
    assert r.returncode == 0 and 'NONFINITE-PIECE-OK' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ----------------------------------------------------------------------------- finite check and Adam skip
ADAM = dict(lr=0.002 * 0.8, beta1=0.9, beta2=0.99 ** 0.8, eps=1e-8)


@pytest.mark.parametrize('n', NC.ADAM_SIZES)
def test_finite_check_flags_every_position_and_only_non_finite_values(n, cuda_device):
    """finite_check_raw: NaN, +inf and -inf at index 0, n - 1, the last element of the vector body and (largest size) in the second grid-stride pass raise
    the flag; all-finite input, FLT_MAX, -FLT_MAX, the smallest subnormal and -0.0 at the same positions do not."""
    from inclusivegan_amd import hip_ops
    rng = np.random.RandomState(n % 9973)
    g = torch.from_numpy(rng.randn(n).astype(np.float32)).to(cuda_device)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    hip_ops.finite_check_raw(g, flag)
    assert int(flag.item()) == 0
    for pos in NC.adam_positions(n):
        keep = g[pos].clone()
        for v in NC.FINITE_SPECIALS:
            g[pos] = v
            flag.zero_()
            hip_ops.finite_check_raw(g, flag)
            assert int(flag.item()) == 0, (n, pos, v)
        for kind, v in NC.KINDS.items():
            g[pos] = float(v)
            flag.zero_()
            hip_ops.finite_check_raw(g, flag)
            assert int(flag.item()) == 1, (n, pos, kind)
        g[pos] = keep
    g[:] = NC.FLT_MAX                       # sums of four FLT_MAX inside the check must not overflow into a false alarm
    flag.zero_()
    hip_ops.finite_check_raw(g, flag)
    assert int(flag.item()) == 0


@pytest.mark.parametrize('n', NC.ADAM_SIZES)
def test_adam_skip_leaves_state_bit_unchanged_and_clear_flag_steps(n, cuda_device):
    """With the flag set (a poison at each position, each kind), w, m, v and both beta powers are bit-unchanged, tail elements included; with the flag
    clear the step equals oracle.optimizer.SimpleAdam as in test_adam_ema_finite_check; ema_raw covers body and tail."""
    from oracle import optimizer as OO
    from inclusivegan_amd import hip_ops
    rng = np.random.RandomState(n % 9973 + 1)
    w0 = rng.randn(n).astype(np.float32)
    wt = torch.from_numpy(w0.copy()).to(cuda_device)
    mt = torch.zeros(n, device=cuda_device); vt = torch.zeros(n, device=cuda_device)
    powt = torch.ones(2, device=cuda_device); flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    adam = OO.SimpleAdam(n, learning_rate=ADAM['lr'], beta1=ADAM['beta1'], beta2=ADAM['beta2'], epsilon=ADAM['eps'])
    wo = w0.copy()

    def step(g):
        gt = torch.from_numpy(g).to(cuda_device)
        flag.zero_()
        hip_ops.finite_check_raw(gt, flag)
        hip_ops.adam_step_raw(wt, gt, mt, vt, ADAM['lr'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], powt, flag)
        return adam.apply(wo, g)

    assert step(rng.randn(n).astype(np.float32))                # a first real step: m, v and the beta powers are non-trivial from here on
    kinds = list(NC.KINDS.items())
    for i, pos in enumerate(NC.adam_positions(n)):
        for j, (kind, v) in enumerate(kinds if n < 100000 else kinds[i % 3:i % 3 + 1]):      # the 2 M-element size: one kind per position, rotating
            before = [t.clone() for t in (wt, mt, vt, powt)]
            g = rng.randn(n).astype(np.float32)
            g[pos] = v
            assert not step(g)
            assert int(flag.item()) == 1, (n, pos, kind)
            for a_, b_ in zip((wt, mt, vt, powt), before):
                assert torch.equal(a_.view(torch.int32), b_.view(torch.int32)), (n, pos, kind)
    g = rng.randn(n).astype(np.float32)
    g[NC.adam_positions(n)[-1]] = NC.FLT_MAX                    # finite: the step is taken (g * g overflows into v on both sides alike)
    with np.errstate(over='ignore'):
        assert step(g) and int(flag.item()) == 0
    g = rng.randn(n).astype(np.float32)
    g[0] = -0.0
    assert step(g) and int(flag.item()) == 0
    fin = np.isfinite(adam.v)
    assert bool((torch.isfinite(vt).cpu().numpy() == fin).all())
    assert rel_err(wt, wo) < 2e-6
    assert rel_err(mt.cpu().numpy()[fin], adam.m[fin]) < 2e-6
    assert rel_err(vt.cpu().numpy()[fin], adam.v[fin]) < 2e-6
    assert abs(float(powt[0]) - float(adam.b1pow)) < 1e-6 and abs(float(powt[1]) - float(adam.b2pow)) < 1e-6
    src = torch.from_numpy(rng.randn(n).astype(np.float32)).to(cuda_device)
    dst0 = wt.clone()
    hip_ops.ema_raw(wt, src, 0.9995)
    assert rel_err(wt, OO.ema(dst0.cpu().numpy(), src.cpu().numpy(), 0.9995)) < 1e-6
    # EMA carries a poison of either side through at its own index only (body, tail and second pass alike)
    for pos in NC.adam_positions(n):
        d = dst0.clone(); s = src.clone()
        (d if pos % 2 else s)[pos] = float('nan')
        hip_ops.ema_raw(d, s, 0.9995)
        bad = ~torch.isfinite(d)
        assert int(bad.sum()) == 1 and bool(bad[pos])


# ----------------------------------------------------------------------------- fused_bias_act: all nine activations, grad 0 / 1 / 2, vector and scalar path
@pytest.mark.parametrize('n', [64, 67], ids=['vector_path', 'scalar_path'])
@pytest.mark.parametrize('act_idx', range(1, 10), ids=['linear', 'relu', 'lrelu', 'tanh', 'sigmoid', 'elu', 'selu', 'softplus', 'swish'])
def test_fused_bias_act_special_values(act_idx, n, cuda_device):
    """fused_bias_act_raw on NaN, +-inf, +-100, +-81, +-79, +-41, +-39, +-0, FLT_MAX, 1e-30 and randn, in x and in ref, against the restated kernel table
    with its range clamps (expRange 80: tanh, sigmoid, softplus, swish; halfExpRange 40: swish' and swish''): the non-finite sets are equal (the oracle's
    taken in fp32, the kernel's format), and the jointly finite values agree to test_fused_bias_act_kernel_table's 1e-5.  The select-based activations
    follow the REFERENCE KERNEL's select, not the framework's relu: relu(NaN) = 0, relu(-inf) = 0, lrelu(NaN) = NaN."""
    from inclusivegan_amd import hip_ops
    x, ref = NC.fba_vectors(n)
    b = np.random.RandomState(act_idx).randn(8).astype(np.float32) if n % 8 == 0 else None      # sizeX % 4 != 0 -> the scalar path, without a bias
    for grad in (0, 1, 2):
        want, o_bad = NC.fba_oracle(x, b, ref if grad else None, grad, act_idx, 0.2, 1.3, 1)
        got = hip_ops.fused_bias_act_raw(_dev(x, cuda_device), _dev(b, cuda_device) if b is not None else None, _dev(ref, cuda_device) if grad else None,
                                         grad, act_idx, 0.2, 1.3, 8 if b is not None else 1, 1).cpu()
        h_bad = ~torch.isfinite(got)
        print('NONFINITE %-10s act %d grad %d n %-3d %-12s oracle %3d  hip %3d  laundered %d  extra %d' % (
            'fba', act_idx, grad, n, 'vector path' if n % 4 == 0 else 'scalar path', int(o_bad.sum()), int(h_bad.sum()), int((o_bad & ~h_bad).sum()), int((h_bad & ~o_bad).sum())))
        assert torch.equal(h_bad, o_bad), (act_idx, grad, torch.nonzero(h_bad != o_bad).flatten().tolist(), x[(h_bad != o_bad).numpy()], ref[(h_bad != o_bad).numpy()])
        # values: the randn part normalised by its maximum as in test_fused_bias_act_kernel_table (the specials would swamp that maximum: they go up to
        # FLT_MAX), each special against its own magnitude, at least 1
        k = len(NC.FBA_SPECIALS)
        both = ~o_bad & torch.isfinite(want.float())
        assert bool(both[k:].all())
        assert float((got.double()[k:] - want[k:]).abs().max() / (want[k:].abs().max() + 1e-30)) < 1e-5, (act_idx, grad)
        sp = both.clone(); sp[k:] = False
        assert bool(((got.double()[sp] - want[sp]).abs() <= 1e-5 * want[sp].abs().clamp(min=1.0)).all()), (act_idx, grad, got[sp].tolist(), want[sp].tolist())
    if act_idx in (2, 3):
        y = hip_ops.fused_bias_act_raw(_dev(np.array([np.nan, -np.inf, np.inf, -1.0], np.float32), cuda_device), None, None, 0, act_idx, 0.2, 2.0, 1, 1).cpu()
        if act_idx == 2:
            assert y.tolist() == [0.0, 0.0, float('inf'), 0.0]
        else:
            assert bool(torch.isnan(y[0])) and y[1:3].tolist() == [float('-inf'), float('inf')]


# ----------------------------------------------------------------------------- max-pool windows
def test_pool_tap_nan_and_inf_windows(cuda_device):
    """PoolTapFn on windows holding one NaN, two NaNs, NaN next to +inf (both orders) and -inf only: forward and routed gradient bit-equal to the framework
    pooling the oracle uses (oracle/lpips.py:27) on the CPU, as test_maxpool_tap_matches_oracle does for ties.  NaN wins, over +inf too (csrc/pool.hip)."""
    from inclusivegan_amd import hip_ops
    x, g_tap, g_pool = NC.pool_input()
    xo = torch.from_numpy(x).requires_grad_(True)
    yo = torch.nn.functional.max_pool2d(xo, 2)
    (gxo,) = torch.autograd.grad([xo * 1.0, yo], [xo], [torch.from_numpy(g_tap), torch.from_numpy(g_pool)])
    xg = to_nhwc_cuda(torch.from_numpy(x), cuda_device).requires_grad_(True)
    tap, yg = hip_ops.PoolTapFn.apply(xg)
    (gxg,) = torch.autograd.grad([tap, yg], [xg], [to_nhwc_cuda(torch.from_numpy(g_tap), cuda_device), to_nhwc_cuda(torch.from_numpy(g_pool), cuda_device)])
    print('NONFINITE %-10s windows: one NaN, two NaNs, NaN next to +inf, -inf only   y oracle %d hip %d   dx oracle %d hip %d' % (
        'pool', int((~torch.isfinite(yo)).sum()), int((~torch.isfinite(yg)).sum()), int((~torch.isfinite(gxo)).sum()), int((~torch.isfinite(gxg)).sum())))
    assert np.array_equal(tap.detach().cpu().numpy(), x, equal_nan=True)
    assert np.array_equal(yg.detach().cpu().numpy(), yo.detach().numpy(), equal_nan=True)
    assert np.array_equal(gxg.cpu().numpy(), gxo.numpy(), equal_nan=True) and bool(torch.isfinite(gxg).all())
