"""CPU: the closed second-order formulas of the style path (hip_ops.StyleGradAllFn's docstring) transcribed in fp64 torch, against autograd through
`style_mod_composite`.  Per layer, s = c_a y.A + b + 1, d = rsqrt(c_w^2 s^2.W2 + 1e-8), W2 = sum_taps w^2; the first-order op maps cotangents (gs, gd) to the
latent gradient dy, and its backward maps one cotangent g on dy to cotangents on (gs, gd, y, A, b, w)."""
import numpy as np
import pytest
import torch

from inclusivegan_amd import hip_ops

CASES = [(3, 32, 12, 8, 3, True), (1, 16, 8, 16, 1, True), (3, 32, 12, 4, 1, False)]      # (N, L, Cin, Cout, k, demodulate)


def closed_first(y, A, b, w, gs, gd, c_a, c_w, demod):
    """dy and the intermediates the backward reuses."""
    s = c_a * (y @ A) + b + 1.0
    if not demod:
        return c_a * (gs @ A.t()), dict(s=s, sigma=gs)
    W2 = (w * w).sum(dim=(0, 1))
    d = torch.rsqrt(c_w * c_w * ((s * s) @ W2) + 1e-8)
    e = -0.5 * c_w * c_w * gd * d ** 3
    m = e @ W2.t()
    sigma = gs + 2.0 * s * m
    return c_a * (sigma @ A.t()), dict(s=s, d=d, e=e, m=m, sigma=sigma, W2=W2)


def closed_second(g, y, A, b, w, gs, gd, c_a, c_w, demod, t):
    """Cotangents on (gs, gd, y, A, b, w) for the cotangent g on dy."""
    v = c_a * (g @ A)
    if not demod:
        return dict(gs=v, A=c_a * (g.t() @ gs))
    s, d, e, m, sigma, W2 = t['s'], t['d'], t['e'], t['m'], t['sigma'], t['W2']
    r = 2.0 * v * s
    eb = r @ W2
    gdb = -0.5 * c_w * c_w * d ** 3 * eb
    qb = 0.75 * c_w * c_w * gd * d ** 5 * eb
    sb = 2.0 * v * m + 2.0 * c_w * c_w * s * (qb @ W2.t())
    W2b = r.t() @ e + c_w * c_w * (s * s).t() @ qb
    return dict(gs=v, gd=gdb, y=c_a * (sb @ A.t()), A=c_a * (g.t() @ sigma) + c_a * (y.t() @ sb), b=sb.sum(dim=0), w=2.0 * w * W2b[None, None])


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('case', CASES)
def test_closed_formulas_match_autograd_of_the_composite(case, monkeypatch):
    N, L, Cin, Cout, k, demod = case
    rng = np.random.RandomState(N * 100 + Cin + Cout)
    mk = lambda *shape: torch.from_numpy(rng.randn(*shape)).requires_grad_(True)
    y, A, w, gs, gd, g = mk(N, L), mk(L, Cin), mk(k, k, Cin, Cout), mk(N, Cin), mk(N, Cout), mk(N, L)
    b = (0.1 * torch.from_numpy(rng.randn(Cin))).requires_grad_(True)
    c_a, c_w = 1.0 / np.sqrt(L), 1.0 / np.sqrt(k * k * Cin)
    # autograd through the composite itself; its two matrix products run on a device only, so they are torch's here
    monkeypatch.setattr(hip_ops, 'matmul', lambda x, w_, alpha=1.0: alpha * (x @ w_))
    s, d = hip_ops.style_mod_composite(y, A, b, w, c_a, c_w, demod)
    outs, gouts = ([s, d], [gs, gd]) if demod else ([s], [gs])
    dy_ref, = torch.autograd.grad(outs, [y], gouts, create_graph=True)
    names = ['gs', 'gd', 'y', 'A', 'b', 'w'] if demod else ['gs', 'A']
    ins = dict(gs=gs, gd=gd, y=y, A=A, b=b, w=w)
    ref = torch.autograd.grad(dy_ref, [ins[n] for n in names], g)
    with torch.no_grad():
        dy, t = closed_first(y, A, b, w, gs, gd, c_a, c_w, demod)
        got = closed_second(g, y, A, b, w, gs, gd, c_a, c_w, demod, t)
    assert rel(dy, dy_ref.detach()) < 1e-12
    for n, r in zip(names, ref):
        assert rel(got[n], r) < 1e-12, n

