"""GPU: the style path differentiated twice through the closed grouped Functions (hip_ops.StyleAllClosedFn / StyleGradAllFn) against an fp64 evaluation
on the CPU, on a three-layer group -- demodulated 3x3, demodulated 1x1, one layer without demodulation -- fed from the latents whole; the same inputs
through the per-layer composite (the path IGAN_STYLE_CLOSED2=0 keeps) as the yardstick of what fp32 gives; and the streaming kernel igan_scale_add.

Metric and bounds are those of tests/test_gpu_ops.py::test_style_mod_fused_vs_oracle for the same quantities: tests.util.rel_err, 2e-5 on the latent
gradient, 1e-4 on the second-order cotangents, 1e-6 absolute where the oracle's is identically zero.  Against the composite: the closed form's deviation is at
most 2 x the composite's, or below FLOOR(K) = 4 sqrt(K) 2^-24 -- every compared quantity is at most four chained fp32 reductions of at most K terms, each
with a rounding error of about sqrt(K) units of 2^-24 relative to the largest element; below that both forms are rounding noise and their ratio is chance."""
import numpy as np
import pytest
import torch

from tests.util import rel_err

pytestmark = pytest.mark.gpu

D, LLAT = 32, 3
FACTOR = 2.0
CASES = [(1, 12, 8, None), (3, 12, 8, None), (1, 36, 20, None), (3, 36, 20, None), (3, 516, 8, None), (3, 12, 8, 0)]      # (N, Cin, Cout, layer whose gd is None)


def _floor(k):
    return 4.0 * np.sqrt(k) * 2.0 ** -24


def _specs(cin, cout):
    """(latent row, Cin, Cout, taps, demodulate): rows 0 and 2 are used (row 2 twice), row 1 by nobody."""
    return [(0, cin, cout, 3, True), (2, cin, cout, 1, True), (2, cin, 3, 1, False)]


def _inputs(N, cin, cout):
    rng = np.random.RandomState(1000 * N + cin + cout)
    specs = _specs(cin, cout)
    f = lambda *shape: torch.from_numpy(rng.randn(*shape))
    data = dict(dlat=f(N, LLAT, D), g=f(N, LLAT, D), layers=[])
    for row, ci, co, k, demod in specs:
        data['layers'].append(dict(A=f(D, ci), b=0.1 * f(ci), w=f(k, k, ci, co), gs=f(N, ci), gd=f(N, co), c_a=1.0 / np.sqrt(D), c_w=1.0 / np.sqrt(k * k * ci)))
    return specs, data


def _leaves(data, dtype, dev):
    mk = lambda t: t.to(dtype).to(dev).requires_grad_(True)
    return mk(data['dlat']), [{k: (mk(v) if torch.is_tensor(v) else v) for k, v in l.items()} for l in data['layers']]


def _second_order(specs, dlat, layers, g, styles, gd_none, third=False):
    """dy = d(sum gs.s + gd.d)/d dlat with create_graph, then the cotangents of <dy, g> on everything.  -> dy, {name: cotangent}."""
    outs, gouts, ins = [], [], dict(dlat=dlat)
    for i, ((s, d), l, spec) in enumerate(zip(styles, layers, specs)):
        outs.append(s); gouts.append(l['gs'])
        ins['A%d' % i], ins['gs%d' % i] = l['A'], l['gs']
        if spec[4]:
            ins['b%d' % i], ins['w%d' % i] = l['b'], l['w']
            if i != gd_none:
                outs.append(d); gouts.append(l['gd'])
                ins['gd%d' % i] = l['gd']
    dy, = torch.autograd.grad(outs, [dlat], gouts, create_graph=True)
    if third:
        return torch.autograd.grad(dy, list(ins.values()), g, create_graph=True, allow_unused=True)
    h = torch.autograd.grad(dy, list(ins.values()), g, allow_unused=True)
    return dy.detach(), dict(zip(ins, h))


def _oracle(specs, data, gd_none):
    dlat, layers = _leaves(data, torch.float64, 'cpu')
    styles = []
    for spec, l in zip(specs, layers):
        s = l['c_a'] * (dlat[:, spec[0]] @ l['A']) + l['b'] + 1.0
        d = torch.rsqrt(l['c_w'] ** 2 * ((s * s) @ (l['w'] * l['w']).sum(dim=(0, 1))) + 1e-8) if spec[4] else None
        styles.append((s, d))
    return _second_order(specs, dlat, layers, data['g'], styles, gd_none)


def _hip_styles(specs, dlat, layers):
    """What networks_stylegan2._precompute_styles does under second_order(): the closed Functions, or the per-layer composites on the unbound rows."""
    from inclusivegan_amd import hip_ops
    ls = [dict(a_w=l['A'], a_b=l['b'], w=l['w'], wsq=hip_ops.sumsq_taps_raw(l['w'].detach()) if spec[4] else None, c_a=l['c_a'], c_w=l['c_w'], demodulate=spec[4])
          for spec, l in zip(specs, layers)]
    res = hip_ops.style_mod_all_closed(ls, dlat, [spec[0] for spec in specs])
    if res is None:
        rows = dlat.unbind(dim=1)
        res = [hip_ops.style_mod_composite(rows[spec[0]], l['a_w'], l['a_b'], l['w'], l['c_a'], l['c_w'], l['demodulate']) for spec, l in zip(specs, ls)]
    return res


def _hip(specs, data, gd_none, dev, closed, monkeypatch, third=False):
    from inclusivegan_amd import hip_ops
    monkeypatch.setattr(hip_ops, '_STYLE_CLOSED2', closed)
    dlat, layers = _leaves(data, torch.float32, dev)
    with hip_ops.second_order():
        styles = _hip_styles(specs, dlat, layers)
    if closed:
        assert styles[0][0].grad_fn.name().startswith('StyleAllClosedFn')
    return _second_order(specs, dlat, layers, data['g'].float().to(dev), styles, gd_none, third=third)


@pytest.mark.parametrize('case', CASES)
def test_closed_style_functions_vs_fp64_and_the_composite(case, cuda_device, monkeypatch):
    N, cin, cout, gd_none = case
    specs, data = _inputs(N, cin, cout)
    dy_o, h_o = _oracle(specs, data, gd_none)
    dy_c, h_c = _hip(specs, data, gd_none, cuda_device, True, monkeypatch)
    dy_p, h_p = _hip(specs, data, gd_none, cuda_device, False, monkeypatch)
    floor = _floor(max(cin, cout, D))
    e_c, e_p = rel_err(dy_c, dy_o), rel_err(dy_p, dy_o)
    print('case %s: dy closed %.2e composite %.2e (floor %.2e)' % (case, e_c, e_p, floor))
    assert float(dy_c[:, 1].abs().max()) == 0.0          # the latent row no layer reads
    bad = []
    if not e_c < 2e-5:
        bad.append('dy: %.2e exceeds 2e-5' % e_c)
    if not e_c <= max(FACTOR * e_p, floor):
        bad.append('dy: closed %.2e > 2 x composite %.2e' % (e_c, e_p))
    for n, ref in h_o.items():
        if ref is None or float(ref.abs().max()) == 0.0:
            assert h_c[n] is None or float(h_c[n].abs().max()) < 1e-6, n
            continue
        assert h_c[n] is not None, n
        e_c, e_p = rel_err(h_c[n], ref), rel_err(h_p[n], ref)
        print('  %-6s closed %.2e composite %.2e' % (n, e_c, e_p))
        if not e_c < 1e-4:
            bad.append('%s: %.2e exceeds 1e-4' % (n, e_c))
        if not e_c <= max(FACTOR * e_p, floor):
            bad.append('%s: closed %.2e > 2 x composite %.2e' % (n, e_c, e_p))
    assert not bad, '\n'.join(bad)


def test_third_differentiation_is_refused(cuda_device, monkeypatch):
    specs, data = _inputs(3, 12, 8)
    with pytest.raises(NotImplementedError):
        _hip(specs, data, None, cuda_device, True, monkeypatch, third=True)


@pytest.mark.parametrize('form', ['both', 'in place', 'no a', 'no b', 'no scales'])
def test_scale_add_vs_torch(form, cuda_device):
    """out = a * alpha[n,c] + b * beta[n,c], channels-last, 36 channels (nine 16-byte lanes: no multiple of 64), three blocks with a ragged tail;
    one multiply-add per element: 1e-6 relative."""
    from inclusivegan_amd import hip_ops
    rng = np.random.RandomState(7)
    N, C, H, W = 2, 36, 13, 13
    t = lambda *shape: torch.from_numpy(rng.randn(*shape)).float().to(cuda_device)
    a, b = t(N, C, H, W).contiguous(memory_format=torch.channels_last), t(N, C, H, W).contiguous(memory_format=torch.channels_last)
    alpha, beta = t(N, C), t(N, C)
    ref = lambda a_, al, b_, be: ((a_.double() * (al.double()[:, :, None, None] if al is not None else 1.0) if a_ is not None else 0.0)
                                  + (b_.double() * (be.double()[:, :, None, None] if be is not None else 1.0) if b_ is not None else 0.0))
    if form == 'both':
        args = (a, alpha, b, beta)
    elif form == 'in place':
        args = (a, None, b, beta)
    elif form == 'no a':
        args = (None, None, b, beta)
    elif form == 'no b':
        args = (a, alpha, None, None)
    else:
        args = (a, None, b, None)
    want = ref(*args)
    got = hip_ops.scale_add_raw(*args, inplace=(form == 'in place'))
    if form == 'in place':
        assert got.data_ptr() == a.data_ptr()
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert rel_err(got, want) <= 1e-6
