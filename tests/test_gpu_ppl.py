"""GPU: perceptual path length.  The endpoint kernel against numpy fp64 (lerp bit for bit, slerp to one fp32 ulp), the crop /
box-mean / range kernel against fp32 and fp64 restatements, the adjacent-pair LPIPS distances against the per-layer Function
on de-interleaved copies, the whole chain (mapping, endpoints, synthesis, crop, VGG, distances, 1 / epsilon^2) per pair
against the fp64 CPU oracle on replayed draws, and the metric harness."""
import numpy as np
import pytest
import torch

from tests.ppl_oracle import FMAP_BASE, RES, oracle_distances

pytestmark = pytest.mark.gpu

EPS = 1e-4
BELOW_ONE = np.nextafter(np.float32(1), np.float32(0))


def positions(n, rng):
    t = rng.rand(n).astype(np.float32)
    t[0] = 0.0
    if n > 1:
        t[-1] = BELOW_ONE
    return t


def run_endpoints(lat, t, mode, dev, misalign=False):
    from inclusivegan_amd import hip_ops
    if misalign:        # a contiguous view that starts 4 bytes into an allocation: the 16-byte path does not apply
        buf = torch.empty(lat.size + 1, device=dev)
        buf[1:] = torch.from_numpy(lat.reshape(-1)).to(dev)
        lat_d = buf[1:].view(lat.shape)
        assert lat_d.data_ptr() % 16 == 4
    else:
        lat_d = torch.from_numpy(lat).to(dev)
    keep = lat_d.clone()
    out = hip_ops.ppl_endpoints_raw(lat_d, torch.from_numpy(t).to(dev), EPS, mode)
    assert out.shape == lat_d.shape and out.dtype == torch.float32
    assert torch.equal(lat_d, keep)                         # lat is unchanged
    return out.cpu().numpy()


@pytest.mark.parametrize('n,dim,misalign', [(3, 7, False), (1, 1, False), (4, 512, False), (4, 512, True), (2, 8 * 512, False), (2, 18 * 512 + 4, False)])
def test_lerp_endpoints_equal_numpy_fp64_bit_for_bit(n, dim, misalign, cuda_device):
    rng = np.random.RandomState(n * 1000 + dim)
    lat = rng.randn(2 * n, dim).astype(np.float32)
    for t in ([positions(n, rng)] if n > 1 else [np.array([0.0], np.float32), np.array([BELOW_ONE], np.float32)]):
        out = run_endpoints(lat, t, 0, cuda_device, misalign)
        a, b = lat[0::2].astype(np.float64), lat[1::2].astype(np.float64)
        t0 = t.astype(np.float64)[:, None]
        e0 = (a + (b - a) * t0).astype(np.float32)
        e1 = (a + (b - a) * (t0 + EPS)).astype(np.float32)
        assert np.array_equal(out[0::2], e0)                # row 2i: the point at t[i]
        assert np.array_equal(out[1::2], e1)                # row 2i + 1: the point at t[i] + epsilon
        if t[0] == 0:
            assert np.array_equal(out[0], lat[0])           # t = 0: a exactly
        assert not np.array_equal(out[0], out[1])


def slerp_fp64(a, b, t):
    from oracle.misc import slerp_np
    return slerp_np(a.astype(np.float64), b.astype(np.float64), t)


@pytest.mark.parametrize('n,dim', [(3, 7), (4, 512), (2, 1024), (2, 1030), (2, 2048)])
def test_slerp_endpoints_within_one_ulp_of_numpy_fp64(n, dim, cuda_device):
    rng = np.random.RandomState(n * 1000 + dim)
    lat = rng.randn(2 * n, dim).astype(np.float32)
    t = positions(n, rng)
    out = run_endpoints(lat, t, 1, cuda_device)
    t0 = t.astype(np.float64)[:, None]
    r0, r1 = slerp_fp64(lat[0::2], lat[1::2], t0), slerp_fp64(lat[0::2], lat[1::2], t0 + EPS)
    ref = np.empty((2 * n, dim), np.float64)
    ref[0::2], ref[1::2] = r0, r1
    ref32 = ref.astype(np.float32)
    ulps = np.abs(out.astype(np.float64) - ref32.astype(np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64)
    print('slerp (%d, %d): max distance from the rounded fp64 result %.2f ulp, %d of %d values differ' % (n, dim, ulps.max(), (ulps > 0).sum(), ulps.size))
    assert ulps.max() <= 1.0
    # the step between the two rows of a pair, which is what the metric measures
    step = out[1::2].astype(np.float64) - out[0::2].astype(np.float64)
    row_ulp = np.spacing(np.abs(ref32).reshape(n, 2, dim).max(axis=(1, 2))).astype(np.float64)[:, None]
    step_err = np.abs(step - (r1 - r0)) / row_ulp
    print('slerp (%d, %d): step error %.2f ulp of the row' % (n, dim, step_err.max()))
    assert step_err.max() <= 2.0
    assert np.abs(np.sqrt((out.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() <= 2.0 ** -22
    # t = 0 is a / |a|
    a0 = lat[0].astype(np.float64)
    assert np.abs(out[0] - (a0 / np.sqrt((a0 * a0).sum())).astype(np.float32)).max() <= np.spacing(np.abs(ref32[0])).max()


CROP_CASES = {       # name: (C, H, W, (y0, y1, x0, x1), factor)
    'whole16_f1': (3, 16, 16, (0, 16, 0, 16), 1),
    'window32_f1': (3, 32, 32, (12, 28, 8, 24), 1),
    'unaligned_f2': (3, 32, 32, (12, 28, 6, 22), 2),
    'whole32x24_f4': (3, 32, 24, (0, 32, 0, 24), 4),
    'one_channel_f1': (1, 32, 32, (12, 28, 8, 24), 1),
    'one_channel_f2': (1, 32, 32, (12, 28, 6, 22), 2),
}


@pytest.mark.parametrize('layout', ['channels_last', 'contiguous'])
@pytest.mark.parametrize('case', sorted(CROP_CASES))
def test_crop_prep(case, layout, cuda_device):
    from inclusivegan_amd import hip_ops
    C, H, W, (y0, y1, x0, x1), f = CROP_CASES[case]
    N = 2
    rng = np.random.RandomState(H * W + f)
    x = rng.uniform(-1.5, 1.5, size=(N, C, H, W)).astype(np.float32)
    xd = torch.from_numpy(x).to(cuda_device)
    if layout == 'channels_last':
        xd = xd.contiguous(memory_format=torch.channels_last)
    keep = xd.clone()
    y = hip_ops.ppl_crop_prep_raw(xd, (y0, y1, x0, x1), f)
    oh, ow = (y1 - y0) // f, (x1 - x0) // f
    assert tuple(y.shape) == (N, C, oh, ow) and y.dtype == torch.float32
    # the layout vgg_features runs on: channel-minor, no copy to get there
    assert tuple(y.stride()) == (oh * ow * C, 1, ow * C, C)
    assert y.contiguous(memory_format=torch.channels_last).data_ptr() == y.data_ptr()
    assert torch.equal(xd, keep)
    got = y.cpu().numpy()
    win = x[:, :, y0:y1, x0:x1]
    if f == 1:
        assert np.array_equal(got, (win + np.float32(1)) * np.float32(127.5))
    else:
        m64 = win.astype(np.float64).reshape(N, C, oh, f, ow, f).mean(axis=(3, 5))
        y64 = (m64 + 1.0) * (255.0 / 2.0)
        err = np.abs(got.astype(np.float64) - y64).max()
        bound = (f * f + 2) * 2.0 ** -24 * 256
        print('crop_prep %s %s: max |y - y64| = %.3e, bound %.3e' % (case, layout, err, bound))
        assert err <= bound
        # the stated order of operations: fp32 sum over rows then columns, one multiply by 1 / f^2, + 1, * 127.5
        s = np.zeros((N, C, oh, ow), np.float32)
        for dy in range(f):
            for dx in range(f):
                s = s + win[:, :, dy::f, dx::f]
        assert np.array_equal(got, (s * np.float32(1.0 / (f * f)) + np.float32(1)) * np.float32(127.5))


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_adjacent_pairs_match_layer_function_on_deinterleaved_copies(cuda_device):
    from inclusivegan_amd import hip_ops
    rng = np.random.RandomState(11)
    shapes = [(64, 16, 16), (128, 8, 8), (256, 4, 4), (512, 2, 2), (512, 1, 1)]
    two_n = 6
    feats = [torch.from_numpy(np.maximum(rng.randn(two_n, *sh), 0).astype(np.float32)).to(cuda_device).contiguous(memory_format=torch.channels_last)
             for sh in shapes]
    lins = [torch.from_numpy((np.abs(rng.randn(sh[0])) / sh[0] / (sh[1] * sh[2])).astype(np.float32)).to(cuda_device) for sh in shapes]
    ptrs = [f.data_ptr() for f in feats]
    d = hip_ops.lpips_adjacent_pairs_raw(feats, lins)
    assert tuple(d.shape) == (two_n // 2,) and [f.data_ptr() for f in feats] == ptrs
    ref = torch.zeros(two_n // 2, device=cuda_device)
    for f, lin in zip(feats, lins):
        ref = ref + hip_ops.LpipsLayerFn.apply(f[0::2].contiguous(memory_format=torch.channels_last),
                                               f[1::2].contiguous(memory_format=torch.channels_last), lin)
    assert float(ref.min()) > 0
    assert rel_err(d, ref) < 1e-6            # the tolerance of test_lpips_pair_table_matches_layer_function
    # the table is cached per (n, device)
    assert hip_ops._lpips_adjacent_tables(3, cuda_device)[0] is hip_ops._lpips_adjacent_tables(3, cuda_device)[0]
    with pytest.raises(ValueError):
        hip_ops.lpips_adjacent_pairs_raw([f[:5] for f in feats], lins)


# ----------------------------------------------------------------------------------------------------------------------
# whole chain

@pytest.fixture(scope='module')
def nets(cuda_device):
    from inclusivegan_amd.dnnlib import tflib
    Gs = tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', seed=1,
                       num_channels=3, resolution=RES, label_size=0, fmap_base=FMAP_BASE, device=cuda_device)
    with torch.no_grad():
        for n, v in Gs.vars.items():
            if n.endswith('noise_strength'):
                v.fill_(0.1)
    lp = {}
    for res in (16, 32):      # VGG input of the cropped / whole image; the same seeded weights
        lp[res] = tflib.Network('lpips', func_name='inclusivegan_amd.metrics.lpips.vgg16_zhang_perceptual', resolution=res, device=cuda_device, seed=1003)
    return Gs, lp


CHAIN_FACTOR = 4        # times the fp32 oracle's own largest per-pair error against fp64


@pytest.mark.parametrize('epsilon', [1e-4, 1e-2])
@pytest.mark.parametrize('space,sampling,crop', [('w', 'full', True), ('w', 'end', True), ('z', 'full', True), ('z', 'end', True), ('w', 'end', False)])
def test_whole_chain_per_pair_against_fp64_oracle(space, sampling, crop, epsilon, nets, cuda_device):
    """Every one of the 8 per-pair distances (two minibatches of 4: the per-minibatch noise redraw is exercised) against the
    fp64 oracle; the bound is CHAIN_FACTOR times what a plain fp32 evaluation of the same oracle loses against fp64."""
    from inclusivegan_amd.dnnlib.tflib import tfutil
    from inclusivegan_amd.metrics.perceptual_path_length import PPL
    Gs, lp = nets
    lpips_net = lp[16 if crop else 32]
    before = {n: v.detach().clone() for n, v in Gs.vars.items()}
    metric = PPL(num_samples=8, epsilon=epsilon, space=space, sampling=sampling, crop=crop, minibatch_per_gpu=4,
                 Gs_overrides=dict(dtype='float32', mapping_dtype='float32'), lpips_net=lpips_net, name='ppl_test')
    rec = tfutil.RecordingRandom()
    with tfutil.use_random(rec):
        d_hip = metric.distances(Gs, num_gpus=1).astype(np.float64)
    assert d_hip.shape == (8,)
    for n, v in Gs.vars.items():
        assert torch.equal(v, before[n]), n                 # the caller's Gs, its noise variables included, is untouched
    t_drawn = np.concatenate([e[1] for e in rec.entries if e[0] == 'uniform'])
    assert t_drawn.shape == (8,) and ((t_drawn == 0).all() if sampling == 'end' else (t_drawn > 0).any())

    g_params = {n: v.detach().double().cpu() for n, v in Gs.vars.items()}
    l_params = {n: v.detach().double().cpu() for n, v in lpips_net.vars.items()}
    d64 = oracle_distances(rec.entries, g_params, l_params, space, crop, epsilon, 4, torch.float64)
    d32 = oracle_distances(rec.entries, g_params, l_params, space, crop, epsilon, 4, torch.float32)
    assert np.isfinite(d64).all() and (d64 > 0).all()
    e32 = np.abs(d32 - d64) / d64
    e_hip = np.abs(d_hip - d64) / d64
    print('ppl chain %s/%s crop=%s eps=%g: fp32 oracle max rel err %.3e, HIP max rel err %.3e, ratio %.3f\n  per pair HIP %s\n  per pair fp32 %s'
          % (space, sampling, crop, epsilon, e32.max(), e_hip.max(), e_hip.max() / e32.max(), np.array2string(e_hip, precision=2), np.array2string(e32, precision=2)))
    assert e_hip.max() <= CHAIN_FACTOR * e32.max()


def test_metric_harness_reports_ppl_wend(nets, cuda_device, capsys):
    from inclusivegan_amd.dnnlib.tflib import tfutil
    from inclusivegan_amd.metrics import metric_base
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    from inclusivegan_amd.metrics.perceptual_path_length import PPL, reject_outliers
    Gs, lp = nets
    args = dict(metric_defaults['ppl_wend'])
    args.update(num_samples=8)
    metric = metric_base.MetricGroup([dict(args, lpips_net=lp[16])]).metrics[0]
    assert type(metric) is PPL
    rec = tfutil.RecordingRandom()
    with tfutil.use_random(rec):
        metric.run(Gs, num_gpus=1)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    value = metric._results[0].value
    assert len(metric._results) == 1 and np.isfinite(value) and value > 0
    assert line.startswith('%-30s' % 'live-network') and line.endswith(('ppl_wend %-10.4f' % value).strip())
    assert line == metric.get_result_str().strip()

    replayed = []
    for _ in range(2):
        tape = tfutil.RandomTape(rec.entries)
        with tfutil.use_random(tape):
            d = metric.distances(Gs, num_gpus=1)
        assert tape.pos == len(rec.entries)
        replayed.append(np.mean(reject_outliers(d)))
    assert replayed[0] == value and replayed[1] == value


def test_small_images_are_rejected_not_worked_around(cuda_device):
    from inclusivegan_amd.dnnlib import tflib
    from inclusivegan_amd.metrics.perceptual_path_length import PPL
    G16 = tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', seed=1,
                        num_channels=3, resolution=16, label_size=0, fmap_base=256, device=cuda_device)
    metric = PPL(num_samples=4, epsilon=1e-4, space='w', sampling='end', crop=True, minibatch_per_gpu=4, Gs_overrides={}, name='ppl_small')
    with pytest.raises(ValueError, match='multiple of 16'):
        metric.distances(G16)
