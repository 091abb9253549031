"""GPU: the fused differentiable-augmentation kernel (csrc/diffaugment.hip) against the fp64 restatement of the contract
(tests/diffaugment_oracle.py, held to two loop-based restatements by tests/test_diffaugment.py), and its wiring into the two
loss functions and the training loop.

Bounds (a priori, not measured): with color |y - y64| <= 64 * 2^-24 * (max |x| of the sample + 1) -- at most ten roundings, each
of a quantity no larger than 6 (max |x| + 1/2) -- and for the transpose the same with max |dy| in the place of max |x| + 1.
Without color outputs are bit copies.  Every position the contract makes zero is exactly 0 under every policy."""
import functools

import numpy as np
import pytest
import torch

from tests import diffaugment_oracle as O
from tests.util import rel_err

pytestmark = pytest.mark.gpu

# the issue's shapes; then two pixels-per-slice boundaries of the colour reduction (1517 pixels: two slices of 759 and 758) and
# the 2- and 4-channel pixel accesses
SHAPES = [(1, 3, 8, 8), (5, 3, 8, 12), (3, 1, 6, 6), (2, 3, 5, 7), (4, 3, 32, 32), (2, 3, 37, 41), (2, 4, 9, 6), (2, 2, 7, 5)]
LARGE = (12, 3, 128, 128)
POLICIES = range(1, 8)
FULL = 'color,translation,cutout'


@functools.lru_cache(maxsize=None)
def case(shape):
    """(x, dy, batches of u) of a shape: built once, shared, never written."""
    x = O.images(shape, seed=sum(shape))
    dy = O.images(shape, seed=sum(shape) + 1)
    batches = O.u_rows(shape[0], seed=shape[2])
    for a in (x, dy, *batches):
        a.setflags(write=False)
    return x, dy, (batches if shape != LARGE else batches[:1])


@functools.lru_cache(maxsize=None)
def reference(shape, batch, bits):
    x, dy, us = case(shape)
    return O.forward64(x, us[batch], bits), O.transpose64(dy, us[batch], bits), O.zero_mask(us[batch], shape, bits)


def run(x, u, bits, dev, transpose=False):
    from inclusivegan_amd import hip_ops
    y = hip_ops.diffaugment_raw(torch.tensor(np.asarray(x)).to(dev), torch.tensor(np.asarray(u)).to(dev), bits, transpose=transpose)
    assert y.is_contiguous(memory_format=torch.channels_last) or y.shape[1] == 1
    return y.cpu().numpy()


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize('shape', SHAPES + [LARGE], ids=str)
def test_forward_and_transpose_against_fp64(cuda_device, shape):
    x, dy, us = case(shape)
    assert shape[0] < 3 or (x[1].min() > 998 and not x[2].any())           # one sample is 1000 + noise, one all zeros
    worst = [0.0, 0.0]
    for k, u in enumerate(us):
        for bits in POLICIES:
            y64, dx64, zero = reference(shape, k, bits)
            y = run(x, u, bits, cuda_device)
            dx = run(dy, u, bits, cuda_device, transpose=True)
            assert not y[zero].any() and bits_equal(y[zero], np.zeros_like(y[zero])), (bits, 'exactly +0 where cut or shifted out')
            if bits & 1:
                ey, edx = np.abs(y - y64), np.abs(dx - dx64)
                worst = [max(worst[0], float((ey / O.bound(x)).max())), max(worst[1], float((edx / np.maximum(O.bound_of(dy, 0.0), 1e-300)).max()))]
                assert (ey <= O.bound(x)).all(), (bits, k, float(ey.max()))
                assert (edx <= O.bound_of(dy, 0.0)).all(), (bits, k, float(edx.max()))
            else:
                assert bits_equal(y, y64.astype(np.float32)), (bits, k)
                assert bits_equal(dx, dx64.astype(np.float32)), (bits, k)
    print('%s: worst error over its a priori bound: forward %.3f, transpose %.3f' % (shape, worst[0], worst[1]))


@pytest.mark.parametrize('shape', [(5, 3, 8, 12), (4, 3, 32, 32), (2, 3, 37, 41), LARGE], ids=str)
def test_adjoint_identity(cuda_device, shape):
    """<T(x1) - T(x2), dy> = <x1 - x2, T' dy> (T is affine: the difference removes the brightness offset), evaluated in fp64 from
    the fp32 outputs, within the forward and transpose bounds combined."""
    x1, dy, us = case(shape)
    x2 = O.images(shape, seed=99)
    u = us[0]
    for bits in POLICIES:
        y1, y2 = run(x1, u, bits, cuda_device).astype(np.float64), run(x2, u, bits, cuda_device).astype(np.float64)
        dx = run(dy, u, bits, cuda_device, transpose=True).astype(np.float64)
        d64, dd = dy.astype(np.float64), x1.astype(np.float64) - x2
        lhs, rhs = ((y1 - y2) * d64).sum(axis=(1, 2, 3)), (dd * dx).sum(axis=(1, 2, 3))
        tol = (np.abs(d64) * (O.bound(x1) + O.bound(x2))).sum(axis=(1, 2, 3)) + (np.abs(dd) * O.bound_of(dy, 0.0)).sum(axis=(1, 2, 3))
        assert (np.abs(lhs - rhs) <= tol).all(), (bits, lhs, rhs, tol)
        assert np.abs(lhs).max() > 0


@pytest.mark.parametrize('shape', [(5, 3, 8, 12), (4, 3, 32, 32), (2, 3, 37, 41), LARGE], ids=str)
def test_same_bits_again_and_for_a_sample_on_its_own(cuda_device, shape):
    x, dy, us = case(shape)
    u = us[0]
    for bits in POLICIES:
        for src, tr in ((x, False), (dy, True)):
            a = run(src, u, bits, cuda_device, transpose=tr)
            assert bits_equal(a, run(src, u, bits, cuda_device, transpose=tr)), (bits, tr, 'second call')
            for k in (range(shape[0]) if shape != LARGE else (0, 7, 11)):
                alone = run(src[k:k + 1], u[k:k + 1], bits, cuda_device, transpose=tr)
                assert bits_equal(alone[0], a[k]), (bits, tr, k, 'a sample of a batch and the same sample alone')


def test_autograd_goes_through_the_transpose_kernel_and_stops_there(cuda_device):
    from inclusivegan_amd import hip_ops
    shape = (4, 3, 32, 32)
    x, dy, us = case(shape)
    u = torch.tensor(us[0]).to(cuda_device)
    dyt = torch.tensor(dy).to(cuda_device)
    for bits in POLICIES:
        xt = torch.tensor(x).to(cuda_device).requires_grad_(True)       # dense NCHW: converted to channels_last like the other ops do
        y = hip_ops.diffaugment(xt, u, bits)
        assert bits_equal(y.detach().cpu().numpy(), run(x, us[0], bits, cuda_device))
        (g,) = torch.autograd.grad(y, [xt], dyt)
        assert bits_equal(g.cpu().numpy(), run(dy, us[0], bits, cuda_device, transpose=True)), bits
    xt = torch.tensor(x).to(cuda_device).requires_grad_(True)
    (g,) = torch.autograd.grad(hip_ops.diffaugment(xt, u, 7), [xt], dyt.requires_grad_(True), create_graph=True)
    with pytest.raises(NotImplementedError, match='second-order'):
        g.sum().backward()
    with pytest.raises(ValueError):
        hip_ops.diffaugment(xt, u, 0)          # the Python side never sends an empty policy to the kernel
    with pytest.raises(NotImplementedError):
        hip_ops.diffaugment(torch.zeros(1, 5, 8, 8, device=cuda_device), u[:1], 7)


def test_capture_into_a_graph_replays_to_the_same_bits(cuda_device):
    from inclusivegan_amd import hip_ops
    shape = (4, 3, 32, 32)
    x, dy, us = case(shape)
    xs, ds = torch.tensor(x).to(cuda_device), torch.tensor(dy).to(cuda_device)
    u = torch.tensor(us[0]).to(cuda_device)
    eager = (hip_ops.diffaugment_raw(xs, u, 7), hip_ops.diffaugment_raw(ds, u, 7, transpose=True))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hip_ops.diffaugment_raw(xs, u, 7)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = (hip_ops.diffaugment_raw(xs, u, 7), hip_ops.diffaugment_raw(ds, u, 7, transpose=True))
    for _ in range(2):
        for t in captured:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[1])
    u.copy_(torch.tensor(us[1]).to(cuda_device))         # a replay reads the draws of ITS iteration
    graph.replay()
    torch.cuda.synchronize()
    assert bits_equal(captured[0].cpu().numpy(), run(x, us[1], 7, cuda_device))


def test_nonfinite_inputs(cuda_device):
    """One NaN (and one infinity) in a kept pixel, in a pixel that is read into a cut position and in one that is shifted out:
    zeros stay exactly 0, without color the value travels to at most its own position, with color it reaches every kept value
    of its sample and nothing of the other sample."""
    shape = (2, 3, 8, 8)
    u = np.stack([np.full(8, O.EDGE_U[2], np.float32), np.full(8, 0.5, np.float32)])      # sample 0: t = (+1, +1), rows and columns 6, 7 cut
    base = O.images(shape, 1)
    base[1] = O.images(shape, 2)[0]                                                       # sample 1: plain noise
    for bad in (np.nan, np.inf):
        for where, copies in (((0, 1, 3, 3), 1), ((0, 1, 7, 7), 0), ((0, 1, 0, 5), 0)):   # kept; lands on the cut (6, 6); row 0 is never read
            x = base.copy()
            x[where] = bad
            clean = run(base, u, 6, cuda_device)
            for bits in POLICIES:
                y = run(x, u, bits, cuda_device)
                zero = O.zero_mask(u, shape, bits)
                assert bits_equal(y[zero], np.zeros_like(y[zero])), (bits, where)
                assert np.isfinite(y[1]).all() and bits_equal(y[1], run(base, u, bits, cuda_device)[1]), (bits, 'the other sample is untouched')
                if bits & 1:
                    assert not np.isfinite(y[0][~zero[0]]).any(), (bits, where)
                else:
                    reached, want = ~np.isfinite(y[0]), O.forward64(x, u, bits)[0]       # the restatement copies: the value sits where it is kept
                    assert np.array_equal(reached, ~np.isfinite(want)) and int(reached.sum()) <= 1, (bits, where)
                    assert bits_equal(np.where(reached, 0, y[0]), np.where(reached, 0, want).astype(np.float32))
                    if bits == 6:
                        assert int(reached.sum()) == copies
            if copies == 0:
                assert bits_equal(run(x, u, 6, cuda_device), clean)


# ---- the loss functions and the loop -------------------------------------------------------------------------------------

def _setup(dev):
    from tests.test_gpu_loop_parity import RES, loop_kwargs
    from tests.test_gpu_networks import _nets
    from inclusivegan_amd.training.dataset import SyntheticDataset
    kw = loop_kwargs(1024, 6)
    B, fmap = kw['sched_args']['minibatch_gpu_base'], kw['G_args']['fmap_base']
    G, D = _nets(dev, fmap=fmap, res=RES)
    ts = SyntheticDataset(resolution=RES, label_size=0, data_size=24, device=dev)
    g = torch.Generator().manual_seed(3)
    reals = (torch.rand(2 * B, 3, RES, RES, generator=g) * 2 - 1).to(dev).contiguous(memory_format=torch.channels_last)
    return G, D, ts, B, reals


@pytest.mark.parametrize('phase', ['loss', 'both', 'reg'])
def test_D_loss_equals_D_on_inputs_augmented_by_the_torch_statement(cuda_device, phase):
    """One draw [fakes + reals, 8] right after the latents (phase 'reg': [reals, 8]); rows 0 .. 2B-1 augment the fakes, the rest the
    reals, in the interleaved one-pass branch ('loss') as in the two-pass branch ('both')."""
    import torch.nn.functional as F
    from inclusivegan_amd.dnnlib.tflib import tfutil
    from inclusivegan_amd.training import augment as A, loss as PL
    dev = cuda_device
    G, D, ts, B, reals = _setup(dev)
    lab2 = torch.zeros(2 * B, 0, device=dev)
    avg0 = G.vars['dlatent_avg'].detach().clone()
    rec = tfutil.RecordingRandom()
    with tfutil.use_random(rec):
        PL.D_logistic_r1(G, D, ts, B, reals, lab2, gamma=100, phase=phase, augment=FULL)
    kinds = [(k, tuple(np.shape(v))) for k, v in rec.entries]
    if phase == 'reg':
        assert kinds == [('uniform', (2 * B, 8))]
        u_at = 0
    else:
        assert kinds[:2] == [('normal', (2 * B, 512)), ('uniform', (4 * B, 8))] and ('uniform', (4 * B, 8)) not in kinds[2:]
        u_at = 1
    with torch.no_grad():
        G.vars['dlatent_avg'].copy_(avg0)
    tape = tfutil.RandomTape(rec.entries)
    with tfutil.use_random(tape):
        loss, reg = PL.D_logistic_r1(G, D, ts, B, reals, lab2, gamma=100, phase=phase, augment=FULL)
    assert tape.pos == len(rec.entries)
    u = torch.tensor(np.asarray(rec.entries[u_at][1])).to(dev)
    with torch.no_grad():
        G.vars['dlatent_avg'].copy_(avg0)
    direct = tfutil.RandomTape([e for i, e in enumerate(rec.entries) if i != u_at])
    with tfutil.use_random(direct), G.derived_scope(), D.derived_scope():
        if phase != 'reg':
            with torch.no_grad():
                fakes = G.get_output_for(tfutil.random_normal([2 * B, 512], dev), lab2, is_training=True)
            fa = A.diffaugment_torch(fakes, u[:2 * B], 7)
            ra = A.diffaugment_torch(reals, u[2 * B:], 7).detach().requires_grad_(True)
            want = F.softplus(D.get_output_for(fa, lab2, is_training=True)[0]) + F.softplus(-D.get_output_for(ra, lab2, is_training=True)[0])
            assert rel_err(loss, want) < 1e-5, phase
        else:
            ra = A.diffaugment_torch(reals, u, 7).detach().requires_grad_(True)
        if phase != 'loss':
            s = D.get_output_for(ra, lab2, is_training=True)[0]
            (gr,) = torch.autograd.grad(s.sum(), [ra], create_graph=True)
            want_reg = (gr * gr).sum(dim=[1, 2, 3]) * 50.0
            assert rel_err(reg, want_reg) < 1e-4, phase         # a squared fp32 gradient norm: the suite's regulariser values are held to 1e-3
    # and the un-augmented function on the same draws gives something else: the keyword reaches D
    with torch.no_grad():
        G.vars['dlatent_avg'].copy_(avg0)
    with tfutil.use_random(tfutil.RandomTape([e for i, e in enumerate(rec.entries) if i != u_at])):
        loss0, reg0 = PL.D_logistic_r1(G, D, ts, B, reals, lab2, gamma=100, phase=phase)
    a, b = (loss, loss0) if phase != 'reg' else (reg, reg0)
    assert rel_err(a, b) > 1e-3


def test_R1_is_taken_on_the_augmented_reals_bit_for_bit(cuda_device):
    """translation,cutout moves bits only, so R1 under the policy IS the un-augmented function fed pre-augmented reals: values and D's
    gradient bucket are bit-identical -- the leaf is made after the augmentation and nothing differentiates the transform."""
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.dnnlib.tflib import tfutil
    from inclusivegan_amd.training import loss as PL
    dev = cuda_device
    G, D, ts, B, reals = _setup(dev)
    lab2 = torch.zeros(2 * B, 0, device=dev)
    u = np.random.RandomState(8).uniform(0, 1, (2 * B, 8)).astype(np.float32)
    out = []
    for policy, feed, tape in (('translation,cutout', reals, [('uniform', u)]),
                               (None, hip_ops.diffaugment_raw(reals, torch.tensor(u).to(dev), 6), [])):
        D.zero_grad(); G.requires_grad_(False)
        src = tfutil.RandomTape(tape)
        with tfutil.use_random(src):
            _, reg = PL.D_logistic_r1(G, D, ts, B, feed, lab2, gamma=100, phase='reg', augment=policy)
        assert src.pos == len(tape)
        torch.autograd.backward(reg.mean(), inputs=list(D.trainables.values()))
        G.requires_grad_(True)
        out.append((reg.detach().clone(), D.flat_grads.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][1].abs().max()) > 0


def test_G_gradient_equals_the_torch_statement_in_place_of_the_kernel(cuda_device, monkeypatch):
    """NN_rec_lpips_weight = 0: the loss is the adversarial term, D(T(G(z))); the draw [B, 8] is the last of the phase.  The gradient of
    every G variable through the transpose kernel against autograd through the torch statement: 5e-3 relative L2 per variable, the
    suite's bound for gradients that pass leaky-ReLU kinks (tests/test_gpu_networks.py)."""
    from inclusivegan_amd.dnnlib.tflib import tfutil
    from inclusivegan_amd.training import augment as A, loss as PL
    dev = cuda_device
    G, D, ts, B, _ = _setup(dev)
    lab = torch.zeros(B, 0, device=dev)
    z = torch.nn.functional.normalize(torch.randn(B, 512, generator=torch.Generator().manual_seed(4)), dim=1).to(dev)
    avg0 = G.vars['dlatent_avg'].detach().clone()

    def step(source, policy):
        with torch.no_grad():
            G.vars['dlatent_avg'].copy_(avg0)
        G.zero_grad(); D.requires_grad_(False)
        with tfutil.use_random(source):
            loss, _ = PL.G_logistic_ns_rec_interp_arb_pathreg(G, D, None, ts, B, None, lab, z, None, lab, z, NN_rec_lpips_weight=0, phase='loss', augment=policy)
        torch.autograd.backward(loss.mean(), inputs=list(G.trainables.values()))
        D.requires_grad_(True)
        return loss.detach().clone(), {n: v.grad.detach().double().clone() for n, v in G.trainables.items() if v.grad is not None}

    rec = tfutil.RecordingRandom()
    loss_hip, g_hip = step(rec, FULL)
    assert rec.entries[-1][0] == 'uniform' and np.shape(rec.entries[-1][1]) == (B, 8)
    assert [k for k, v in rec.entries if np.shape(v) == (B, 8)] == ['uniform']
    calls = []
    monkeypatch.setattr(A, 'augment', lambda x, u, bits: (calls.append(bits), A.diffaugment_torch(x, u, bits))[1])
    tape = tfutil.RandomTape(rec.entries)
    loss_torch, g_torch = step(tape, FULL)
    assert calls == [7] and tape.pos == len(rec.entries)
    assert rel_err(loss_hip, loss_torch) < 1e-5
    assert set(g_hip) == set(g_torch) and len(g_hip) > 10
    for n in g_hip:
        if g_torch[n].numel() > 1 and float(g_torch[n].norm()) > 0:
            e = float((g_hip[n] - g_torch[n]).norm() / g_torch[n].norm())
            assert e < 5e-3, (n, e)
    loss_off, _ = step(tfutil.RandomTape(rec.entries[:-1]), None)
    assert rel_err(loss_hip, loss_off) > 1e-3


def test_training_loop_with_the_full_policy_graph_replay_equals_eager_bitwise(cuda_device, monkeypatch):
    """The nine iterations of test_graph_replay_equals_eager_bitwise with the full policy in both loss dictionaries: the captured
    ops (the augmentation's draws and launches inside them) are faithful, every op's loss and digests and the final weights are
    bit-identical with graphs on and off, and the policy really reaches the ops: the first D and G steps differ from the policy-off run."""
    from inclusivegan_amd.dnnlib import EasyDict
    from tests.test_gpu_loop_parity import flat_of, loop_kwargs, record_loop

    def kwargs(policy):
        extra = {} if policy is None else dict(augment=policy)
        return loop_kwargs(1024, 6, data_size=48, label=dict(label_size=10, label_kind='onehot'),
                           G_loss_args=EasyDict(func_name='training.loss.G_logistic_ns_rec_interp_arb_pathreg', NN_rec_lpips_weight=2.5, **extra),
                           D_loss_args=EasyDict(func_name='training.loss.D_logistic_r1', gamma=100, **extra))
    runs = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('IGAN_HIP_GRAPHS', mode)
        runs[mode] = record_loop(9, kwargs(FULL), reseed=4242, tap=False, keep_state='digest')
    off = record_loop(1, kwargs(None), reseed=4242, tap=False, keep_state='digest')       # eager, one iteration: enough to see the difference
    a, b = runs['1'], runs['0']
    assert a['graphs'] is not None and a['graphs']['faithful'] and all(c['faithful'] for c in a['graphs']['checks']) and b['graphs'] is None
    assert [o['name'] for o in a['ops']] == [o['name'] for o in b['ops']]
    assert {o['name'] for o in a['ops']} == {'G', 'G_reg', 'D', 'D_reg'}
    for x, y in zip(a['ops'], b['ops']):
        assert x['value'] == y['value'], (x['name'], x['it'], x['value'], y['value'])
        assert x['digest'] == y['digest'], (x['name'], x['it'])
    for k in ('G', 'D', 'Gs', 'dlatent_avg', 'G_pow', 'D_pow'):
        assert np.array_equal(a['final'][k], b['final'][k]), k
    assert a['final']['pl_mean'] == b['final']['pl_mean']
    d0 = flat_of(a['init'], 'D')
    assert float(np.abs(a['final']['D'][:d0.size] - d0).max()) > 0         # the bucket is padded past the last variable
    first = lambda log, name: [o for o in log['ops'] if o['name'] == name][0]
    for name in ('G', 'D'):
        assert first(b, name)['digest'][0] != first(off, name)['digest'][0], name          # the gradient bucket of the first step
    assert first(b, 'D')['digest'][2] != first(off, 'D')['digest'][2]                       # D's weights after its first step
