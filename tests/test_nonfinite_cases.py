"""CPU: the condition on the non-finite cases (tests/nonfinite_cases.py), from the oracle side only, and the pins of the oracle pieces the GPU
tests lean on.  For every case: the clean oracle is finite; the poison reaches some output; every output that is checked for values keeps at
least 75 % of its elements finite (otherwise the value assertion checks nothing); the declared unreachable set is finite and equal to the clean
result; a declared reach does not overlap it.  Needs only the oracle and NumPy / PyTorch on the CPU."""
import numpy as np
import pytest
import torch

from tests import nonfinite_cases as NC

CASES = NC.all_cases()


def test_case_ids_are_unique_and_every_family_is_present():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    assert {c.op for c in CASES} == {'ban', 'upfirdn', 'firban', 'conv', 'modconv', 'cba', 'style', 'mbstd', 'lpips'}
    for c in CASES:
        assert c.poison[2] in NC.KINDS


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_oracle_side_condition(case):
    NC.check_oracle_side(case)


def test_conv_poisons_are_interior_and_centre_tap():
    """Every tap of the weight gradient meets the poisoned pixel, and the poisoned filter entry is the centre tap (no output sees it through the
    padding only): then the oracle's set is exactly the channel / the window, which is what the cases' masks assume."""
    for cfg in NC.CONVS + [NC.CONV_PIECE]:
        _name, n, cin, h, w, cout, k = cfg[:7]
        p = dict(NC.conv_poisons(cfg))
        r = k // 2
        for inp in ('x', 'dy'):
            _n, _c, ph, pw = p[inp]
            assert (h == 1 and w == 1) or (r <= ph < h - r and r <= pw < w - r), (cfg, inp)
        assert p['w'][:2] == (r, r)
    case = [c for c in CASES if c.op == 'conv' and c.cfg is NC.CONVS[0] and c.poison[0] == 'x' and c.poison[2] == 'nan'][0]
    want = case.want()
    _n, c, ph, pw = case.poison[1]
    bad = NC.nonfinite32(want['dw'])
    assert bool(bad[:, :, c, :].all()) and int(bad.sum()) == 9 * 40
    bad = NC.nonfinite32(want['y'])
    assert int(bad.sum()) == 9 * 40 and bool(bad[1, :, ph - 1:ph + 2, pw - 1:pw + 2].all())


def test_zero_extended_reach_contains_the_oracle_set_and_is_4x4():
    for case in CASES:
        if case.op == 'upfirdn' and case.reach is not None:
            want = case.want()
            shapes = {k: tuple(v.shape) for k, v in want.items()}
            _un, rc = case.masks(shapes)
            (name, m), = rc.items()
            bad = NC.nonfinite32(want[name]).numpy()
            assert (bad <= m).all() and bad.sum() == case.cfg[5] ** 2 and m.sum() <= 16 and m.sum() > bad.sum()


def test_kernel_restatement_selects_and_clamps():
    """oracle.fused_bias_act.fused_bias_act_kernel_ref at the values where the outcome is the reference kernel's decision, not IEEE arithmetic:
    the selects (a comparison with NaN is false) and the range clamps, in fp32 and fp64."""
    from oracle.fused_bias_act import fused_bias_act_kernel_ref as K
    nan, inf = float('nan'), float('inf')
    for dt in (torch.float32, torch.float64):
        v = lambda *a: torch.tensor(a, dtype=dt)
        one = lambda a: float(a[0])
        # relu(NaN) = 0, relu(-inf) = 0, relu(+inf) = inf; lrelu(NaN) = NaN, lrelu(-inf) = -inf
        assert K(v(nan, -inf, inf), None, None, 0, 2, 0.0, 2.0, 1).tolist() == [0.0, 0.0, inf]
        y = K(v(nan, -inf, -1.0), None, None, 0, 3, 0.2, 2.0, 1)
        assert np.isnan(one(y)) and float(y[1]) == -inf and abs(float(y[2]) + 0.4) < 1e-6
        # gradient forms select on ref = y / gain: ref = NaN takes the else arm
        assert K(v(3.0, 3.0), None, v(nan, 1.0), 1, 2, 0.0, 2.0, 1).tolist() == [0.0, 6.0]
        y = K(v(3.0, 3.0), None, v(nan, 1.0), 1, 3, 0.25, 2.0, 1)
        assert y.tolist() == [1.5, 6.0]
        # tanh / sigmoid / softplus / swish clamps at +-80, swish' and swish'' at 40
        assert K(v(-100.0, 100.0, -inf, inf, -81.0, 81.0), None, None, 0, 4, 0.0, 1.0, 1).tolist() == [-1.0, 1.0, -1.0, 1.0, -1.0, 1.0]
        assert K(v(-100.0, -inf, -81.0), None, None, 0, 5, 0.0, 1.0, 1).tolist() == [0.0, 0.0, 0.0]
        assert K(v(81.0, 100.0, inf), None, None, 0, 8, 0.0, 1.0, 1).tolist() == [81.0, 100.0, inf]
        assert K(v(-81.0, -100.0, -inf), None, None, 0, 9, 0.0, 1.0, 1).tolist() == [0.0, 0.0, 0.0]      # not -inf * 0
        assert K(v(2.0, 2.0, 2.0), None, v(41.0, 100.0, inf), 1, 9, 0.0, 1.0, 1).tolist() == [2.0, 2.0, 2.0]
        assert K(v(2.0, 2.0, 2.0), None, v(41.0, 100.0, inf), 2, 9, 0.0, 1.0, 1).tolist() == [0.0, 0.0, 0.0]
        for act in (4, 5, 8, 9):
            assert np.isnan(one(K(v(nan), None, None, 0, act, 0.0, 1.0, 1)))
        # inside the range the clamps change nothing
        x = torch.linspace(-79.0, 79.0, 317, dtype=dt)
        assert torch.equal(K(x, None, None, 0, 4, 0.0, 1.0, 1), torch.tanh(x))
        assert torch.equal(K(x, None, None, 0, 9, 0.0, 1.0, 1), x * torch.sigmoid(x))
    # the unclamped fp32 formula would be inf / inf at 100: what the clamp is for
    c = torch.exp(torch.tensor(100.0)); d = 1.0 / c
    assert np.isnan(float((c - d) / (c + d)))


def test_fba_vectors_and_oracle_mask():
    """The special-value vector holds every value the issue lists, in x and in ref, for a vector-path size and a scalar-path size; the oracle's
    non-finite set is the fp32 one (tanh'' at ref = FLT_MAX overflows in fp32, not in fp64)."""
    for n in (64, 67):
        x, ref = NC.fba_vectors(n)
        assert x.shape == ref.shape == (n,)
        for vec in (x, ref):
            s = vec[:len(NC.FBA_SPECIALS)]
            assert np.isnan(s).sum() == 1 and (s == np.inf).sum() == 1 and (s == -np.inf).sum() == 1 and np.signbit(s[s == 0]).sum() == 1
            for val in (100, 81, 79, 41, 39):
                assert (s == val).sum() == 1 and (s == -val).sum() == 1
            assert (s == np.float32(NC.FLT_MAX)).sum() == 1 and (s == np.float32(1e-30)).sum() == 1
    y64, bad = NC.fba_oracle(np.array([1.0, 0.0], np.float32), None, np.array([NC.FLT_MAX, NC.FLT_MAX], np.float32), 1, 4, 0.0, 1.0, 1)
    assert bool(torch.isfinite(y64).all()) and bad.tolist() == [True, True]


def test_adam_sizes_and_positions():
    n = NC.ADAM_TWO_PASS
    assert n in NC.ADAM_SIZES and n % 4 == 3 and n // 4 > 2048 * 256           # a second grid-stride pass and a scalar tail both exist
    pos = NC.adam_positions(n)
    assert pos[0] == 0 and pos[-1] == n - 1 and (n // 4) * 4 - 1 in pos and any(2048 * 256 * 4 <= p < (n // 4) * 4 - 1 for p in pos)
    assert NC.adam_positions(1) == [0] and NC.adam_positions(5) == [0, 3, 4] and NC.adam_positions(4) == [0, 3]
    for v in NC.FINITE_SPECIALS:
        assert np.isfinite(np.float32(v))
    assert np.float32(NC.FINITE_SPECIALS[2]) > 0 and np.float32(NC.FINITE_SPECIALS[2]) < np.finfo(np.float32).tiny


def test_pool_reference_windows():
    """The framework pooling the oracle uses lets NaN win over everything, +inf included, and routes the gradient to one element per window."""
    x, _g_tap, g_pool = NC.pool_input()
    xo = torch.from_numpy(x).requires_grad_(True)
    y = torch.nn.functional.max_pool2d(xo, 2)
    c = 3
    yd = y.detach()
    assert all(np.isnan(float(yd[0, c, i, j])) for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)))
    assert float(yd[0, c, 3, 3]) == -np.inf and np.isfinite(float(yd[0, c, 2, 2]))
    (g,) = torch.autograd.grad(y, xo, torch.from_numpy(g_pool))
    assert bool(torch.isfinite(g).all())
    assert int((g[0, c] != 0).sum()) <= 16 and bool(((g[0, c].reshape(4, 2, 4, 2) != 0).sum(dim=(1, 3)) <= 1).all())


def _pick(op, cfg_name, inp, kind='nan'):
    return [c for c in CASES if c.op == op and c.name == cfg_name and c.poison[0] == inp and c.poison[2] == kind][0]


def test_shared_assertions_bite():
    """check_outputs() on stand-ins for the HIP side: the oracle's own results rounded to fp32 pass; a laundered value, a changed bit in the
    unreachable set, a non-finite element outside the declared reach and a wrong finite value each fail."""
    case = _pick('conv', NC.CONVS[0][0], 'x')
    want = case.want()
    good = {k: v.float() for k, v in want.items()}
    clean = {k: v.float() for k, v in case.want(False).items()}
    NC.check_outputs(case, want, good, clean)
    n, c, ph, pw = case.poison[1]

    def mutated(name, index, value):
        bad = {k: v.clone() for k, v in good.items()}
        bad[name][index] = value
        return bad

    with pytest.raises(AssertionError, match='laundered'):
        NC.check_outputs(case, want, mutated('dw', (0, 0, c, 0), 0.0), clean)
    with pytest.raises(AssertionError, match='spread'):
        NC.check_outputs(case, want, mutated('y', (0, 0, 0, 0), float(good['y'][0, 0, 0, 0]) * (1 + 2e-7) + 1e-12), clean)
    with pytest.raises(AssertionError, match='spread|outside'):
        NC.check_outputs(case, want, mutated('dw', (0, 0, c - 1, 0), float('nan')), clean)
    with pytest.raises(AssertionError):
        NC.check_outputs(case, want, mutated('dx', (0, 0, 0, 0), float('inf')), clean)
    # a wrong value where the poison may reach but the oracle stays finite: only the value check can see it
    cba = _pick('cba', NC.CBA[0], 'x')
    w2 = cba.want()
    g2 = {k: v.float() for k, v in w2.items()}
    c2 = {k: v.float() for k, v in cba.want(False).items()}
    NC.check_outputs(cba, w2, g2, c2)
    bad = {k: v.clone() for k, v in g2.items()}
    bad['db'][0] *= 1.01
    with pytest.raises(AssertionError):
        NC.check_outputs(cba, w2, bad, c2)
    # the zero-extended FIR: the 4x4 footprint is allowed, one element further is not
    fir = _pick('upfirdn', 'fir4 3x3 taps', 'x', '+inf')
    w3 = fir.want()
    g3 = {k: v.float() for k, v in w3.items()}
    c3 = {k: v.float() for k, v in fir.want(False).items()}
    m, iy, ix, ch = fir.poison[1]
    inside = {k: v.clone() for k, v in g3.items()}
    inside['y'][m, iy + 1 - 3, ix + 1 - 3, ch] = float('nan')
    NC.check_outputs(fir, w3, inside, c3)
    outside = {k: v.clone() for k, v in g3.items()}
    outside['y'][m, iy, ix + 1 + 1, ch] = float('nan')               # reach: ox in [ix + 1 - 3, ix + 1]
    with pytest.raises(AssertionError, match='spread|outside'):
        NC.check_outputs(fir, w3, outside, c3)
    exact = _pick('upfirdn', 'fir4 4x4 taps', 'x')
    w4 = exact.want()
    g4 = {k: v.float() for k, v in w4.items()}
    m, iy, ix, ch = exact.poison[1]
    g4['y'][m, iy + 1 - 3, ix + 1 - 4, ch] = float('nan')          # one column left of the 4x4 filter's own set
    with pytest.raises(AssertionError):
        NC.check_outputs(exact, w4, g4, {k: v.float() for k, v in exact.want(False).items()})
