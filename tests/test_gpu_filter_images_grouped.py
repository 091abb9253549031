"""GPU: the grouped filter image (igan_filter_images_grouped) and the per-op filter image scope built on it (hip_ops.FilterImageScope).

Everything here is an equality of bytes: a filter image is a per-channel maximum (exact, order-free) and an element-wise split, and a convolution that is
handed an image reads exactly what it would have written for itself."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TAPS = 9


@pytest.fixture(scope='module')
def env():
    from inclusivegan_amd import _abi, hip_ops
    lib = _abi.get_plugin()
    if lib.igan_conv_piece_form() != 2:
        pytest.skip('the grouped filter image belongs to the two-piece fp16 form (the default)')
    return _abi, hip_ops, lib, torch.device('cuda', 0)


def _launches(lib, reset=True):
    n = ctypes.c_ulonglong(0)
    assert lib.igan_debug_filter_image_launches(ctypes.byref(n), 1 if reset else 0) == 0
    return int(n.value)


def _filter(cin, cout, wt, seed):
    """Seeded filter in the call's layout (HWIO [tap][k][n], or [tap][n][k] when transposed) with the planted output channels."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(TAPS, cin, cout, generator=g) * torch.exp(4.0 * torch.randn(1, 1, cout, generator=g))     # [tap][k][n]; channel magnitudes over e^+-8
    w[:, :, 1:4] = torch.randn(TAPS, cin, 3, generator=g)          # (the planted maxima below stand far above these)
    w[:, :, 0] = 0.0                                    # an all-zero output channel
    w[TAPS - 1, cin - 1, 1] = 3.0e4                     # the maximum is the LAST (tap, k) element ...
    w[0, 0, 2] = 3.0e4                                  # ... the FIRST
    w[4, 5, 3] = -3.0e4                                 # a negative maximum
    w[:, :, 5] = torch.randn(TAPS, cin, generator=g) * 1e-40     # a subnormal-only channel
    w[3, 7, 5] = 0.0
    if wt:
        w = w.permute(0, 2, 1)
    return w.contiguous()


def _compared_bytes(cin, cout):
    return 4 * TAPS * cin * cout + 4 * cout             # the pieces [K/16][tap][n][2][16] and inv[Nn]: what a convolution call reads


def _single(env, w, cin, cout, wt):
    _abi, hip_ops, lib, dev = env
    nbytes = int(lib.igan_filter_image_bytes(3, 3, cin, cout))
    assert nbytes >= _compared_bytes(cin, cout)
    out = torch.full((nbytes,), 0xA5, device=dev, dtype=torch.uint8)
    _abi.check(lib.igan_filter_image(None, ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(out.data_ptr()), 3, 3, cin, cout, 1 if wt else 0))
    return out[:_compared_bytes(cin, cout)]


def _grouped(env, entries):
    """entries: (w on the device, cin, cout, wt) -> the compared bytes of each, written by ONE grouped call into one arena."""
    _abi, hip_ops, lib, dev = env
    sizes = [int(lib.igan_filter_image_bytes(3, 3, cin, cout)) for _, cin, cout, _ in entries]
    offs, total = [], 0
    for s in sizes:
        offs.append(total)
        total += (s + 255) // 256 * 256
    arena = torch.full((total,), 0x5A, device=dev, dtype=torch.uint8)
    assert arena.data_ptr() % 16 == 0
    arr = (_abi.FilterImageDesc * len(entries))()
    for d, (w, cin, cout, wt), off in zip(arr, entries, offs):
        d.w, d.out, d.KH, d.KW, d.Cin, d.Cout, d.w_transposed = w.data_ptr(), arena.data_ptr() + off, 3, 3, cin, cout, 1 if wt else 0
    _launches(lib)
    _abi.check(lib.igan_filter_images_grouped(None, arr, len(entries)))
    assert _launches(lib) == 2
    return [arena[off:off + _compared_bytes(cin, cout)] for (w, cin, cout, wt), off in zip(entries, offs)], arena


CASES = [(128, 128, False), (128, 128, True), (256, 128, False), (256, 128, True), (128, 512, False), (1024, 128, False)]


@pytest.fixture(scope='module')
def singles(env):
    dev = env[3]
    entries = [(_filter(cin, cout, wt, 100 + i).to(dev), cin, cout, wt) for i, (cin, cout, wt) in enumerate(CASES)]
    return entries, [_single(env, *e) for e in entries]


def test_grouped_equals_single(env, singles):
    entries, want = singles
    got, _ = _grouped(env, entries)
    for (w, cin, cout, wt), a, b in zip(entries, got, want):
        assert torch.equal(a, b), (cin, cout, wt, int((a != b).sum()))
    # the planted channels did what they were planted for: 1 / S of the zero and the subnormal-only channel is the smallest the form has, 2^-113 ... and
    # the three 3e4 channels share one exponent
    inv = got[0][4 * TAPS * 128 * 128:].view(torch.float32)
    assert inv[0] == inv[5] and inv[1] == inv[2] == inv[3] and inv[1] > inv[0]


def test_reversed_order_gives_the_same_bytes(env, singles):
    entries, want = singles
    got, _ = _grouped(env, entries[::-1])
    for (w, cin, cout, wt), a, b in zip(entries[::-1], got, want[::-1]):
        assert torch.equal(a, b), (cin, cout, wt)


def test_count_one_and_count_max(env, singles):
    _abi = env[0]
    entries, want = singles
    got, _ = _grouped(env, entries[2:3])
    assert torch.equal(got[0], want[2])
    many = [entries[i & 1] for i in range(_abi.FILTER_MAX_GROUPS)]       # both orientations of the smallest filter, alternating
    got, _ = _grouped(env, many)
    for i, a in enumerate(got):
        assert torch.equal(a, want[i & 1]), i


def _conv(env, x, w, cin, cout, wt, image=None):
    """3x3, stride 1, SAME on x [1, 32, 32, cin] (channel-minor) through the C ABI; `image`: the filter image handed over as w_pieces."""
    _abi, hip_ops, lib, dev = env
    y = torch.empty((1, 32, 32, cout), device=dev)
    p = _abi.Conv2DParams(x=x.data_ptr(), w=w.data_ptr(), y=y.data_ptr(), in_scale=None, out_scale=None, workspace=None, workspace_floats=0,
                          N=1, H=32, W=32, Cin=cin, OH=32, OW=32, Cout=cout, KH=3, KW=3, stride=1, up=1, pad_y=1, pad_x=1,
                          w_transposed=1 if wt else 0, splits=1, alpha=1.0, bias=None, act=0, act_alpha=0.0, act_gain=1.0)
    splits, sliced, wsf = ctypes.c_int(1), ctypes.c_int(0), ctypes.c_size_t(0)
    _abi.check(lib.igan_conv2d_plan(ctypes.byref(p), ctypes.byref(splits), ctypes.byref(sliced), ctypes.byref(wsf)))
    ws = torch.empty((max(wsf.value, 1),), device=dev)
    if wsf.value:
        p.workspace, p.workspace_floats = ws.data_ptr(), wsf.value
    if splits.value > 1:
        p.splits, p.sliced_tiles = splits.value, sliced.value
    if image is not None:
        p.w_pieces, p.w_pieces_bytes = image.data_ptr(), int(lib.igan_filter_image_bytes(3, 3, cin, cout))
    buf = ctypes.create_string_buffer(128)
    _abi.check(lib.igan_conv2d_kernel_name(ctypes.byref(p), buf, 128))
    assert buf.value.decode().startswith('conv_fwd_planes'), buf.value
    _abi.check(lib.igan_conv2d(None, ctypes.byref(p)))
    return y


@pytest.mark.parametrize('cin,cout,wt', [(128, 128, False), (256, 128, True)], ids=['C128->128 forward', 'C128->256 data gradient'])
def test_convolution_through_a_grouped_image(env, cin, cout, wt):
    _abi, hip_ops, lib, dev = env
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 32, 32, cin, generator=g).to(dev)
    w = _filter(cin, cout, wt, 9).to(dev)
    other = _filter(128, 128, False, 10).to(dev)            # a neighbour in the same grouped call
    _, arena = _grouped(env, [(other, 128, 128, False), (w, cin, cout, wt)])
    off = (int(lib.igan_filter_image_bytes(3, 3, 128, 128)) + 255) // 256 * 256
    _launches(lib)
    got = _conv(env, x, w, cin, cout, wt, image=arena[off:])
    assert _launches(lib) == 0
    want = _conv(env, x, w, cin, cout, wt)
    assert _launches(lib) == 2
    assert torch.equal(got, want)


class _TwoLayers:
    """ConvBiasActFn -> ModConvBanFn, 128 channels, N = 1, 32 x 32; the weights are views into one flat bucket, as a network's are."""

    def __init__(self, env, seed=3):
        _abi, hip_ops, lib, dev = env
        self.hip_ops = hip_ops
        g = torch.Generator().manual_seed(seed)
        n = TAPS * 128 * 128
        self.flat = (torch.randn(2 * n, generator=g) / (TAPS * 128) ** 0.5).to(dev)
        self.w1 = self.flat[:n].view(3, 3, 128, 128).requires_grad_()
        self.w2 = self.flat[n:].view(3, 3, 128, 128).requires_grad_()
        self.x = torch.randn(1, 128, 32, 32, generator=g).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
        self.b1 = (0.1 * torch.randn(128, generator=g)).to(dev).requires_grad_()
        self.b2 = (0.1 * torch.randn(128, generator=g)).to(dev)
        self.s = (torch.rand(1, 128, generator=g) + 0.5).to(dev).requires_grad_()
        self.d = (torch.rand(1, 128, generator=g) + 0.5).to(dev)
        self.noise = torch.randn(1, 1, 32, 32, generator=g).to(dev)
        self.strength = torch.tensor(0.1, device=dev)
        self.t = torch.randn(1, 128, 32, 32, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        self.geom = hip_ops.ConvGeom(3, 3, 1, 1, 1, 1)
        # state of the raw optimizer kernel
        self.grad = (0.05 * torch.randn(2 * n, generator=g)).to(dev)
        self.m, self.v = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.pow = torch.ones(2, device=dev)
        self.flag = torch.zeros(1, device=dev, dtype=torch.int32)
        self.other = (torch.randn(2 * n, generator=g) / (TAPS * 128) ** 0.5).to(dev)

    def __call__(self):
        ops = self.hip_ops
        h = ops.ConvBiasActFn.apply(self.x, self.w1, self.b1, self.geom, (32, 32), 3, 0.2, 2.0 ** 0.5)
        y = ops.ModConvBanFn.apply(h, self.w2, self.s, self.d, self.b2, self.noise, self.strength, self.geom, (32, 32), 3, 0.2, 2.0 ** 0.5)
        grads = torch.autograd.grad((y * self.t).sum(), [self.x, self.w1, self.w2, self.b1, self.s])
        return (y.detach(),) + tuple(grads)

    def change_weights(self, how):
        """In-place through the raw kernels: no tensor's version counter moves."""
        before = (self.w1._version, self.w2._version, self.flat._version)
        if how == 'adam':
            self.hip_ops.adam_step_raw(self.flat, self.grad, self.m, self.v, 0.05, 0.0, 0.99, 1e-8, self.pow, self.flag)
        else:
            self.hip_ops.ema_raw(self.flat, self.other, 0.5)
        assert before == (self.w1._version, self.w2._version, self.flat._version)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


IMAGING_CALLS = 4       # both layers' forward and data-gradient calls take the piece form at 1 024 rows; the weight gradients image no filter


def test_scope_equals_no_scope(env):
    _abi, hip_ops, lib, dev = env
    op = _TwoLayers(env)
    _launches(lib)
    want = [t.clone() for t in op()]
    assert _launches(lib) == 2 * IMAGING_CALLS
    scope = hip_ops.FilterImageScope('test')
    rec = [t.clone() for t in scope.run(op)]                # the recording pass images per call
    assert _launches(lib) == 2 * IMAGING_CALLS and scope.state == 'recorded' and len(scope.recorded) == IMAGING_CALLS
    got = [t.clone() for t in scope.run(op)]
    assert _launches(lib) == 2 and scope.state == 'ready'
    assert _same(rec, want) and _same(got, want)
    again = scope.run(op)                                   # nothing was dropped after the first prepared pass: every entry had its consumer
    assert _launches(lib) == 2 and len(scope.slices) == IMAGING_CALLS and _same(again, want)
    assert hip_ops._filter_scope is None                    # left with the op


def test_nothing_is_kept_between_executions(env):
    _abi, hip_ops, lib, dev = env
    op = _TwoLayers(env)
    scope = hip_ops.FilterImageScope('test')
    scope.run(op)
    first = [t.clone() for t in scope.run(op)]
    for how in ('adam', 'ema'):
        op.change_weights(how)
        _launches(lib)
        got = [t.clone() for t in scope.run(op)]
        assert _launches(lib) == 2
        want = op()
        assert _same(got, want), how
        assert not torch.equal(got[0], first[0])            # the weights did change


def test_replay_follows_the_weights(env):
    _abi, hip_ops, lib, dev = env
    from inclusivegan_amd.dnnlib.tflib import graphs
    op = _TwoLayers(env)
    step = graphs.GraphedStep(op, enabled=True, eager_calls=1, name='filter_scope_test')
    step()                                                  # eager: records
    assert step.filter_scope.state == 'recorded'
    for i, how in enumerate((None, 'adam', 'ema')):
        if how is not None:
            op.change_weights(how)
        torch.cuda.synchronize()
        out = step()                                        # first time: capture + replay; then replays
        torch.cuda.synchronize()
        assert step.graph is not None and step.filter_scope.state == 'ready'
        got = [t.clone() for t in out]
        want = op()                                         # eager, no scope, same state
        assert _same(got, want), (i, how)
    assert step.replays == 3
