"""GPU: the inference surface on the device -- igan_images_to_uint8 / igan_images_from_uint8 through hip_ops and tflib,
Network.run with transforms and its staged copies, run_generator.generate_images and run_metrics.run end to end.

The yardstick is never the kernel itself: it is the torch statement of the reference's conversion evaluated ON THE CPU
(`cpu_statement` below, the body metrics/metric_base.py had before it delegated) or fp64 NumPy."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def cpu_statement(images, drange=(-1, 1), nchw_to_nhwc=False, shrink=1):
    images = images.detach().cpu().to(torch.float32)
    if shrink > 1:
        images = torch.nn.functional.avg_pool2d(images, shrink, shrink)
    if nchw_to_nhwc:
        images = images.permute(0, 2, 3, 1)
    scale = 255 / (drange[1] - drange[0])
    images = images * scale + (0.5 - drange[0] * scale)
    return images.clamp(0, 255).to(torch.uint8).contiguous().numpy()


def boundary_values():
    """fp32 (k - 128) / 127.5 for k = 0 .. 255 with its neighbours at -2, -1, +1, +2 ulp: where images that were uint8 once live,
    and where a contracted multiply-add gives another byte than a multiply and an add."""
    centre = np.array([(k - 128) / 127.5 for k in range(256)], dtype=np.float32)
    bits = centre.view(np.int32)
    out = []
    for d in (-2, -1, 0, 1, 2):
        step = np.where(centre >= 0, d, -d).astype(np.int32)        # towards larger values for d > 0 on both sides of zero
        nb = (bits + step).view(np.float32).copy()
        if d != 0:
            zero = centre == 0
            nb[zero] = np.nextafter(np.float32(0), np.float32(np.sign(d)), dtype=np.float32) * abs(d)
        out.append(nb)
    return np.stack(out, 1).reshape(-1)                             # 1280 values


def chunks(values, shape):
    """The values cut into tensors of `shape` (the last one wraps around)."""
    per = int(np.prod(shape))
    n = -(-len(values) // per)
    flat = np.resize(values, n * per)
    return [torch.from_numpy(flat[i * per:(i + 1) * per].reshape(shape).copy()) for i in range(n)]


def test_boundary_vectors_tell_a_fused_multiply_add_apart():
    """CPU-side premise of the bit-for-bit tests: on these inputs one rounding (fp64 product and sum, exact, then fp32) and the
    CPU statement's two roundings give different bytes at least once."""
    v = boundary_values()
    two = cpu_statement(torch.from_numpy(v).reshape(1, 1, 1, -1)).reshape(-1)
    fused = np.clip((v.astype(np.float64) * 127.5 + 128.0).astype(np.float32), 0, 255).astype(np.uint8)
    assert (two != fused).sum() >= 1


@pytest.mark.parametrize('C', [1, 3, 4, 5])
def test_boundary_vectors_bit_for_bit(cuda_device, C):
    from inclusivegan_amd import hip_ops
    v = boundary_values()
    for W in (1, 4, 7, 9):
        for x in chunks(v, (2, C, 5, W)):
            for nhwc in (False, True):
                got = hip_ops.images_to_uint8(x.to(cuda_device), (-1, 1), nhwc, 1)
                assert got.dtype == torch.uint8 and got.is_contiguous()
                assert tuple(got.shape) == ((2, 5, W, C) if nhwc else (2, C, 5, W))
                assert np.array_equal(got.cpu().numpy(), cpu_statement(x, nchw_to_nhwc=nhwc)), (C, W, nhwc)


@pytest.mark.parametrize('C,W', [(3, 9), (4, 4), (1, 7), (5, 4)])
def test_input_layouts_give_the_same_bytes(cuda_device, C, W):
    from inclusivegan_amd import hip_ops
    dev = cuda_device
    for x in chunks(boundary_values(), (2, C, 5, W)):
        x = x.to(dev)
        for nhwc in (False, True):
            want = cpu_statement(x, nchw_to_nhwc=nhwc)
            assert np.array_equal(hip_ops.images_to_uint8(x, (-1, 1), nhwc, 1).cpu().numpy(), want)
            cl = x.contiguous(memory_format=torch.channels_last)
            big = torch.full((2, C, 6, W + 1), 7.0, device=dev)
            big[:, :, 1:, 1:] = x
            view = big[:, :, 1:, 1:]                     # odd offset: no 16-byte alignment
            wide = torch.full((2, C, 5, 2 * W), -7.0, device=dev)
            wide[..., ::2] = x
            strided = wide[..., ::2]                     # stride_w = 2
            assert view.stride(3) == 1 and view.storage_offset() % 4 != 0 and strided.stride(3) == 2
            for name, t in (('channels_last', cl), ('offset view', view), ('stride_w 2', strided)):
                assert torch.equal(t, x)
                assert np.array_equal(hip_ops.images_to_uint8(t, (-1, 1), nhwc, 1).cpu().numpy(), want), (name, nhwc)


@pytest.mark.parametrize('shrink', [2, 4])
def test_shrink_is_exact_on_exactly_summable_inputs(cuda_device, shrink):
    """Multiples of 2^-10 in [-1.25, 1.25]: every box sum is exact in any order, so the bytes equal the CPU statement's."""
    from inclusivegan_amd import hip_ops
    rng = np.random.RandomState(shrink)
    x = torch.from_numpy((rng.randint(-1280, 1281, size=(4, 3, 24, 24)) / 1024.0).astype(np.float32))
    for nhwc in (False, True):
        want = cpu_statement(x, nchw_to_nhwc=nhwc, shrink=shrink)
        big = torch.zeros(4, 3, 25, 25, device=cuda_device)
        big[:, :, 1:, 1:] = x.to(cuda_device)
        for t in (x.to(cuda_device), x.to(cuda_device).contiguous(memory_format=torch.channels_last), big[:, :, 1:, 1:]):
            assert torch.equal(t.cpu(), x)
            got = hip_ops.images_to_uint8(t, (-1, 1), nhwc, shrink)
            assert tuple(got.shape) == tuple(want.shape) and np.array_equal(got.cpu().numpy(), want), (shrink, nhwc, t.stride())


def test_shrink_drops_the_remainder(cuda_device):
    from inclusivegan_amd import hip_ops
    rng = np.random.RandomState(7)
    x = torch.from_numpy((rng.randint(-1280, 1281, size=(2, 3, 7, 7)) / 1024.0).astype(np.float32))
    for nhwc in (False, True):
        got = hip_ops.images_to_uint8(x.to(cuda_device), (-1, 1), nhwc, 2)
        assert tuple(got.shape) == (2, 3, 3, 3)
        assert np.array_equal(got.cpu().numpy(), cpu_statement(x, nchw_to_nhwc=nhwc, shrink=2))
        assert np.array_equal(got.cpu().numpy(), cpu_statement(x[:, :, :6, :6], nchw_to_nhwc=nhwc, shrink=2))


def _excused(got, x, shrink):
    """Number of bytes that differ from floor(v64) -- each of them by 1 and only where v64 is within 1e-4 of an integer."""
    n, c, h, w = x.shape
    oh, ow = h // shrink, w // shrink
    x64 = x.numpy().astype(np.float64)[:, :, :oh * shrink, :ow * shrink]
    v64 = x64.reshape(n, c, oh, shrink, ow, shrink).mean(axis=(3, 5)) * 127.5 + 128.0
    want = np.clip(np.floor(v64), 0, 255).astype(np.int64)
    diff = got.astype(np.int64) - want
    off = diff != 0
    assert np.all(np.abs(diff[off]) == 1), 'a byte is off by more than 1'
    assert np.all(np.abs(v64[off] - np.round(v64[off])) < 1e-4), 'a byte differs where v64 is not within 1e-4 of an integer'
    return int(off.sum())


@pytest.mark.parametrize('shrink', [2, 3, 4])
def test_shrink_against_fp64(cuda_device, shrink):
    """uniform(-1.2, 1.2): the box sums round, so a byte may differ from fp64 only on the edge of an integer.  The cap of 1e-3 of
    the elements is a condition, not a measurement (about 2e-4 of them lie that near an integer); the CPU statement is held to it too."""
    from inclusivegan_amd import hip_ops
    rng = np.random.RandomState(1234)
    x = torch.from_numpy(rng.uniform(-1.2, 1.2, size=(4, 3, 24, 24)).astype(np.float32))
    got = hip_ops.images_to_uint8(x.to(cuda_device), (-1, 1), False, shrink).cpu().numpy()
    n_gpu = _excused(got, x, shrink)
    n_cpu = _excused(cpu_statement(x, shrink=shrink), x, shrink)
    big = torch.from_numpy(rng.uniform(-1.2, 1.2, size=(4, 3, 64, 64)).astype(np.float32))
    n_cpu_big = _excused(cpu_statement(big, shrink=shrink), big, shrink)
    print('shrink %d: excused kernel %d / %d, CPU statement %d / %d and %d / %d' % (shrink, n_gpu, got.size, n_cpu, got.size, n_cpu_big, big.numel() // shrink ** 2))
    assert n_gpu <= 1e-3 * got.size and n_cpu <= 1e-3 * got.size and n_cpu_big <= 1e-3 * (big.numel() // shrink ** 2)
    nhwc = hip_ops.images_to_uint8(x.to(cuda_device), (-1, 1), True, shrink).cpu().numpy()
    assert np.array_equal(nhwc, got.transpose(0, 2, 3, 1))


def test_saturation_and_non_finite(cuda_device):
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.dnnlib import tflib
    x = torch.tensor([-np.inf, -3.0, -1.0, 1.0, 3.0, np.inf, np.nan], dtype=torch.float32).reshape(1, 1, 1, 7)
    want = [0, 0, 0, 255, 255, 255, 0]                  # 1 * 127.5 + 128 = 255.5 saturates; NaN is DEFINED as 0 here
    for nhwc in (False, True):
        assert hip_ops.images_to_uint8(x.to(cuda_device), (-1, 1), nhwc, 1).cpu().reshape(-1).tolist() == want
    assert tflib.convert_images_to_uint8(x.to(cuda_device).expand(2, 3, 1, 7), nchw_to_nhwc=True).cpu()[1, 0, :, 2].tolist() == want
    # through the box sum: {-inf, -3} -> -inf -> 0;  {-1, 1} -> 0 -> 128;  {3, +inf} -> +inf -> 255;  the seventh column is dropped
    assert hip_ops.images_to_uint8(x.to(cuda_device).expand(1, 1, 2, 7), (-1, 1), False, 2).cpu().reshape(-1).tolist() == [0, 128, 255]


def test_argument_errors(cuda_device):
    from inclusivegan_amd import hip_ops
    x = torch.zeros(2, 3, 4, 4, device=cuda_device)
    for bad in (dict(shrink=0), dict(shrink=5), dict(drange=(1, 1)), dict(drange=(0, float('inf'))), dict(drange=(1,))):
        kw = dict(drange=(-1, 1), nchw_to_nhwc=False, shrink=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            hip_ops.images_to_uint8(x, **kw)
    with pytest.raises(ValueError):
        hip_ops.images_to_uint8(x[0], (-1, 1), False, 1)
    with pytest.raises(TypeError):
        hip_ops.images_to_uint8(x.double(), (-1, 1), False, 1)
    with pytest.raises(RuntimeError):
        hip_ops.images_to_uint8(x.cpu(), (-1, 1), False, 1)
    with pytest.raises(TypeError):
        hip_ops.images_from_uint8(x, (-1, 1), False)
    with pytest.raises(ValueError):
        hip_ops.images_from_uint8(torch.zeros(2, 3, 4, dtype=torch.uint8, device=cuda_device), (-1, 1), False)


@pytest.mark.parametrize('C', [1, 3])
def test_images_from_uint8_bit_for_bit(cuda_device, C):
    from inclusivegan_amd import hip_ops
    for u in chunks(np.arange(256, dtype=np.uint8), (2, C, 3, 5)):
        want = (u.to(torch.float32) * ((1 - -1) / 255) + -1).numpy()                 # the CPU statement (tfutil.py:249-252)
        assert np.array_equal(want, np.float32(u.numpy()) * np.float32(2 / 255) + np.float32(-1))
        got = hip_ops.images_from_uint8(u.to(cuda_device), (-1, 1), False)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, C, 3, 5) and np.array_equal(got.cpu().numpy(), want)
        nhwc = u.permute(0, 2, 3, 1).contiguous()
        got = hip_ops.images_from_uint8(nhwc.to(cuda_device), (-1, 1), True)
        assert tuple(got.shape) == (2, C, 3, 5) and np.array_equal(got.cpu().numpy(), want)
        got = hip_ops.images_from_uint8(u.to(cuda_device), (0, 255), False)
        assert np.array_equal(got.cpu().numpy(), u.to(torch.float32).numpy())


# ---- Network.run ------------------------------------------------------------------------------------------------------------

RES, FMAP = 16, 512


@pytest.fixture(scope='module')
def nets(cuda_device):
    from inclusivegan_amd.dnnlib import tflib
    kw = dict(num_channels=3, resolution=RES, label_size=0, fmap_base=FMAP, device=cuda_device)
    G = tflib.Network('G', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', seed=41, **kw)
    D = tflib.Network('D', func_name='inclusivegan_amd.training.networks_stylegan2.D_stylegan2_feature', architecture='resnet', seed=42, **kw)
    rng = np.random.RandomState(0)
    with torch.no_grad():       # noise strengths are zero-initialised; make the noise matter
        for n, v in G.vars.items():
            if n.endswith('noise_strength'):
                v.copy_(torch.from_numpy(np.asarray(rng.randn(*v.shape) * 0.1, dtype=np.float32)).to(cuda_device).reshape(v.shape))
    Gs = G.clone('Gs')
    return G, D, Gs


def _images_from_uint8(images, labels):
    from inclusivegan_amd.dnnlib import tflib
    return [tflib.convert_images_from_uint8(images), labels]


def test_run_with_transforms_and_staging(cuda_device, nets):
    from inclusivegan_amd.dnnlib import tflib
    G, D, Gs = nets
    dev = cuda_device
    z = np.random.RandomState(5).randn(5, 512)
    splits = [(0, 2), (2, 4), (4, 5)]

    def direct(b, e):
        with torch.no_grad():
            return Gs.get_output_for(torch.as_tensor(z[b:e].astype(np.float32)).to(dev), torch.zeros(e - b, 0, device=dev), randomize_noise=False)

    plain = np.concatenate([direct(b, e).cpu().numpy() for b, e in splits])
    bytes_ = np.concatenate([cpu_statement(direct(b, e), nchw_to_nhwc=True) for b, e in splits])
    Gs._run_staging = None
    got = Gs.run(z, None, minibatch_size=2, randomize_noise=False, output_transform=dict(func=tflib.convert_images_to_uint8, nchw_to_nhwc=True))
    assert got.dtype == np.uint8 and got.shape == (5, RES, RES, 3) and np.array_equal(got, bytes_)
    assert Gs._run_staging['uses'] == [2, 1]
    again = Gs.run(z, None, minibatch_size=2, randomize_noise=False, output_transform=dict(func=tflib.convert_images_to_uint8, nchw_to_nhwc=True))
    assert np.array_equal(again, bytes_) and Gs._run_staging['uses'] == [4, 2]          # both pinned buffers were reused
    # no transforms: get_output_for's values bit for bit, None == zeros
    got = Gs.run(z, None, minibatch_size=2, randomize_noise=False)
    assert got.dtype == np.float32 and np.array_equal(got, plain)
    assert np.array_equal(Gs.run(z, np.zeros([5, 0]), minibatch_size=2, randomize_noise=False), got)
    assert np.array_equal(Gs.run(z, None, randomize_noise=False, minibatch_size=5, num_gpus=1, assume_frozen=True, print_progress=False),
                          direct(0, 5).cpu().numpy())
    as_list = Gs.run(z, None, minibatch_size=2, randomize_noise=False, return_as_list=True)
    assert isinstance(as_list, list) and len(as_list) == 1 and np.array_equal(as_list[0], plain)
    with pytest.raises(TypeError, match='output_transform'):
        Gs.run(z, None, out_mul=127.5)
    # input transform: uint8 images into D
    u = np.random.RandomState(6).randint(0, 256, size=(5, 3, RES, RES)).astype(np.uint8)
    floats = np.float32(u) * np.float32(2 / 255) + np.float32(-1)
    a = D.run(u, None, minibatch_size=2, input_transform=dict(func=_images_from_uint8))
    b = D.run(floats, None, minibatch_size=2)
    assert isinstance(a, tuple) and len(a) == len(b) == D.num_outputs == 2 and a[1] is None and b[1] is None      # features are off by default
    assert a[0].shape[0] == 5 and np.array_equal(a[0], b[0])
    a = D.run(u, None, minibatch_size=2, input_transform=dict(func=_images_from_uint8), return_features=True)
    b = D.run(floats, None, minibatch_size=2, return_features=True)
    assert all(p.shape[0] == 5 and np.array_equal(p, q) for p, q in zip(a, b))


def test_metric_generate_path_is_unchanged(cuda_device, nets):
    from inclusivegan_amd.metrics.metric_base import DummyMetric
    _G, _D, Gs = nets
    m = DummyMetric(name='dummy')
    torch.manual_seed(99)
    floats = m._generate(Gs, 4, dict(is_validation=True), as_uint8=False)
    torch.manual_seed(99)
    got = m._generate(Gs, 4, dict(is_validation=True))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, 3, RES, RES)
    assert np.array_equal(got.cpu().numpy(), cpu_statement(floats))


# ---- the two CLIs end to end ------------------------------------------------------------------------------------------------

def _classify(images):
    """A fixed stand-in for the Inception softmax: uint8 images [n, C, H, W] -> probabilities [n, 7]."""
    assert images.dtype == torch.uint8
    x = images.to(torch.float32).reshape(images.shape[0], -1) / 255.0
    proj = torch.randn(x.shape[1], 7, generator=torch.Generator().manual_seed(3)).to(x.device) / 8.0
    return torch.softmax(x @ proj, dim=1)


def test_generate_images_and_run_metrics_end_to_end(cuda_device, nets, tmp_path, monkeypatch):
    import PIL.Image
    from inclusivegan_amd import pretrained_networks, run_generator, run_metrics
    from inclusivegan_amd.dnnlib import EasyDict, tflib
    from inclusivegan_amd.metrics.inception_score import IS
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    from inclusivegan_amd.training import misc
    pkl = str(tmp_path / 'network-snapshot-000001.pkl')
    misc.save_pkl(nets, pkl)

    def files(run_dir):
        return {f: open(os.path.join(run_dir, f), 'rb').read() for f in sorted(os.listdir(run_dir))}

    runs = []
    for name in ('a', 'b'):
        torch.manual_seed(77)
        run_generator.generate_images(pkl, num_images=4, minibatch_size=2, run_dir=str(tmp_path / name))
        runs.append(files(str(tmp_path / name)))
    assert list(runs[0]) == ['%06d.png' % i for i in range(4)] and runs[0] == runs[1]
    decoded = [np.asarray(PIL.Image.open(os.path.join(str(tmp_path / 'a'), f))) for f in runs[0]]
    assert all(d.shape == (RES, RES, 3) and d.dtype == np.uint8 for d in decoded)

    Gs = pretrained_networks.load_networks(pkl)[-1]
    assert Gs is pretrained_networks.load_networks(pkl)[-1]
    noise_vars = [v for n, v in Gs.components.synthesis.vars.items() if n.startswith('noise')]
    assert len(noise_vars) == 2 * 3 - 1                 # 4x4 .. 16x16
    torch.manual_seed(77)
    rnd = np.random.RandomState(0)
    want = []
    for _ in range(2):
        z = rnd.randn(2, 512)
        tflib.set_vars({v: rnd.randn(*v.shape) for v in noise_vars})
        want += list(Gs.run(z, None, output_transform=dict(func=tflib.convert_images_to_uint8, nchw_to_nhwc=True), randomize_noise=True))
    assert all(np.array_equal(d, w) for d, w in zip(decoded, want))
    assert len({d.tobytes() for d in decoded}) == 4

    # run_metrics: a tiny inception-score entry, the classifier injected
    monkeypatch.setitem(metric_defaults, 'is_tiny', EasyDict(name='is_tiny', func_name='metrics.inception_score.IS', num_images=16, num_splits=2, minibatch_per_gpu=4))
    run_dir = str(tmp_path / 'results' / '00000-run-metrics')
    torch.manual_seed(5)
    run_metrics.run(pkl, ['is_tiny'], dataset=None, data_dir=None, mirror_augment=False, run_dir=run_dir, inject=dict(classify_fn=_classify, feature_fn=None))
    lines = open(os.path.join(run_dir, 'metric-is_tiny.txt')).read().splitlines()
    direct = IS(name='is_tiny', num_images=16, num_splits=2, minibatch_per_gpu=4, classify_fn=_classify)
    torch.manual_seed(5)
    direct.run(Gs, log_results=False)
    mean, std = (r.value for r in direct._results)
    assert len(lines) == 1 and lines[0].startswith('%-30s time ' % 'network-snapshot-000001')
    assert lines[0].endswith(('is_tiny_mean %-10.4f is_tiny_std %-10.4f' % (mean, std)).rstrip())
    assert mean > 1.0
    with pytest.raises(RuntimeError, match='classify_fn'):
        run_metrics.run(pkl, ['is_tiny'], dataset=None, data_dir=None, mirror_augment=False)
