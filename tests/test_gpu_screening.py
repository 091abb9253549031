"""GPU: the screening interval of the exact searches (csrc/exact_distance.h nn1_tol) held to fp64 on the adversarial row families of
tests/screening_cases.py, per product family, and the four consumers end to end on the same rows.

(a) igan_nn1_update runs with a `dots` tensor the test owns; rho = |a - d2_exact| / t is computed on the host from the
    products read back (screening_cases.interval_use) and must stay <= RHO_BAR = 0.5 for EVERY pair.  The screen is sound while
    rho <= 1; the factor of two is for the rows the few thousand sampled pairs do not see.  Which GEMM family a product lands
    on depends on (nq, nc, dim, alignment) and each family has its own summation order, so every test asserts the family with
    igan_conv2d_kernel_name on the parameters distance_products() builds: the coverage cannot rot when the dispatch moves.
(b) flat, flat_u8, flat_noisy and positive rows through nn1, nnk (k = 1, 10), the manifold radii + membership (kcap 4) and the
    k-means step: indices, labels and membership EQUAL to the brute force (duplicates to the lower index), distances to the
    bars of the consumers' own tests (1e-12 * max for the searches, RTOL = 1e-11 for the k-means step), two batch orders of
    nnk bit-identical.  The k-means step takes dim <= 4096 and <= 64 centres: it runs at dim 3072 and 768 on the 128x32 tile.

One fp64 reference per (family, dim), shared by every shape cut out of it (screening_cases.cut)."""
import ctypes

import numpy as np
import pytest
import torch

import screening_cases as S

pytestmark = pytest.mark.gpu

RHO_BAR = 0.5
DIMS = (768, 3072, 12288, 49152)

# name: (nq, nc, dims, float offset of the query view, the kernel igan_conv2d_kernel_name must report)
SHAPES = {
    'dense_small': (16, 136, DIMS, 0, 'dense_small_kernel<16, true>'),
    'dma': (72, 136, DIMS, 0, 'conv_fwd_dma_kernel<true, false>'),
    'vec_no_walk': (72, 136, (3076,), 0, 'conv_fwd_kernel<128, 128, 2, 4, true, true, false>'),
    'scalar_odd_dim': (72, 136, (3073,), 0, 'conv_fwd_kernel<128, 128, 2, 4, true, false, false>'),
    'scalar_view': (72, 136, (3072, 12288), 2, 'conv_fwd_kernel<128, 128, 2, 4, true, false, false>'),
    'tile_128x64': (72, 40, DIMS, 0, 'conv_fwd_kernel<128, 64, 4, 2, true, true, false>'),
    'tile_128x32': (72, 20, DIMS, 0, 'conv_fwd_kernel<128, 32, 4, 1, true, true, false>'),
    'tile_32x128': (24, 136, (3073,), 0, 'conv_fwd_kernel<32, 128, 1, 4, true, false, false>'),
    'thin_out': (72, 3, (512,), 0, 'thin_out_kernel<1>'),
}


def _dev(a, dev, offset=0):
    """The rows on the device, contiguous; offset = 2 floats puts them 8 bytes off 16-byte alignment."""
    buf = torch.empty(a.size + 4, device=dev, dtype=torch.float32)
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))          # a copy: the shared case is read-only
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
    return view


def product_kernel(qd, cd, dots):
    """The kernel distance_products() (csrc/exact_distance.h) launches for these operands: the same igan_conv2d_params."""
    from inclusivegan_amd import _abi
    nq, dim = qd.shape
    p = _abi.Conv2DParams(x=qd.data_ptr(), w=cd.data_ptr(), y=dots.data_ptr(), in_scale=None, out_scale=None, workspace=None, workspace_floats=0,
                          N=nq, H=1, W=1, Cin=dim, OH=1, OW=1, Cout=cd.shape[0], KH=1, KW=1, stride=1, up=1, pad_y=0, pad_x=0, w_transposed=1,
                          splits=1, alpha=1.0, bias=None, act=0, act_alpha=0.0, act_gain=1.0)
    buf = ctypes.create_string_buffer(128)
    _abi.check(_abi.get_plugin().igan_conv2d_kernel_name(ctypes.byref(p), buf, 128))
    return buf.value.decode()


def _operands(dev, shape, family, dim):
    nq, nc, _, offset, kernel = SHAPES[shape]
    q, c, ans = S.cut(family, nq, nc, dim)
    qd, cd = _dev(q, dev, offset), _dev(c, dev)
    dots = torch.full((nq, nc), float('nan'), device=dev, dtype=torch.float32)
    assert product_kernel(qd, cd, dots) == kernel, (shape, product_kernel(qd, cd, dots))
    return q, c, ans, qd, cd, dots


# ----------------------------------------------------------------------------- (a) the interval, per product family
@pytest.mark.parametrize('family', S.FAMILIES)
@pytest.mark.parametrize('shape,dim', [(s, d) for s in SHAPES for d in SHAPES[s][2]])
def test_interval_holds_the_exact_distance(cuda_device, shape, dim, family):
    from inclusivegan_amd import _abi, hip_ops
    q, c, ans, qd, cd, dots = _operands(cuda_device, shape, family, dim)
    nq, nc = dots.shape
    qn, cn = hip_ops.row_sqnorm_raw(qd), hip_ops.row_sqnorm_raw(cd)
    best_d2, best_idx = hip_ops.nn1_state(nq, cuda_device)
    _abi.check(_abi.get_plugin().igan_nn1_update(hip_ops._stream(), hip_ops._ptr(qd), hip_ops._ptr(qn), hip_ops._ptr(cd), hip_ops._ptr(cn),
                                                 hip_ops._ptr(best_d2), hip_ops._ptr(best_idx), hip_ops._ptr(dots), nq, nc, dim, 0))
    got = dots.cpu().numpy()
    assert np.isfinite(got).all()
    rho = S.interval_use(q, c, got, qn.cpu().numpy(), cn.cpu().numpy(), d2=ans['d2'])
    old = S.interval_use(q, c, got, qn.cpu().numpy(), cn.cpu().numpy(), d2=ans['d2'], tol=S.statistical_tol)
    print('rho %-14s %-10s dim %5d  worst %.4f  (of the statistical interval 2^-22 sqrt(dim): %.4f)' % (shape, family, dim, rho.max(), old.max()))
    assert rho.max() <= RHO_BAR, (shape, family, dim, float(rho.max()))


# ----------------------------------------------------------------------------- (b) the consumers on the same rows
FLAT_LIKE = ('flat', 'flat_u8', 'flat_noisy', 'positive')
END_TO_END = [(s, 12288, f) for s in ('dma', 'tile_128x32') for f in FLAT_LIKE] + [('dma', 49152, 'flat')]
KMEANS = [('tile_128x32', d, f) for d in (3072, 768) for f in FLAT_LIKE]


def _distances_close(d2_got, d2_want):
    got, want = np.sqrt(d2_got), np.sqrt(d2_want)
    err = float(np.abs(got - want).max())
    print('largest distance error %.3e, bar %.3e' % (err, 1e-12 * want.max()))
    assert err <= 1e-12 * want.max()


@pytest.mark.parametrize('shape,dim,family', END_TO_END)
def test_nn1_on_adversarial_rows(cuda_device, shape, dim, family):
    from inclusivegan_amd import hip_ops
    q, c, ans, qd, cd, _ = _operands(cuda_device, shape, family, dim)
    qn, cn = hip_ops.row_sqnorm_raw(qd), hip_ops.row_sqnorm_raw(cd)
    d2, idx = hip_ops.nn1_state(q.shape[0], cuda_device)
    hip_ops.nn1_update_raw(qd, qn, cd, cn, d2, idx, 0)
    assert np.array_equal(idx.cpu().numpy(), ans['nn_idx'])
    _distances_close(d2.cpu().numpy(), ans['knn_d2'][:, 0])


@pytest.mark.parametrize('shape,dim,family', END_TO_END)
def test_nnk_on_adversarial_rows(cuda_device, shape, dim, family):
    from inclusivegan_amd import hip_ops
    q, c, ans, qd, cd, _ = _operands(cuda_device, shape, family, dim)
    nq, nc = q.shape[0], c.shape[0]
    qn, cn = hip_ops.row_sqnorm_raw(qd), hip_ops.row_sqnorm_raw(cd)
    for k in (1, 10):
        states = []
        for batches in (((0, nc),), ((nc // 2, nc), (0, nc // 2))):
            d2, idx = hip_ops.nnk_state(nq, k, cuda_device)
            for b0, b1 in batches:
                hip_ops.nnk_update_raw(qd, qn, cd[b0:b1], cn[b0:b1], d2, idx, b0)
            states.append((d2, idx))
        assert np.array_equal(states[0][1].cpu().numpy(), ans['knn_idx'][:, :k]), k
        _distances_close(states[0][0].cpu().numpy(), ans['knn_d2'][:, :k])
        assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1]), k      # bits included


@pytest.mark.parametrize('shape,dim,family', END_TO_END)
def test_manifold_on_adversarial_rows(cuda_device, shape, dim, family):
    from inclusivegan_amd import hip_ops
    q, c, ans, qd, cd, _ = _operands(cuda_device, shape, family, dim)
    nq, nc = q.shape[0], c.shape[0]
    qn, cn = hip_ops.row_sqnorm_raw(qd), hip_ops.row_sqnorm_raw(cd)
    kth = hip_ops.knn_radius_state(nq, 4, cuda_device)
    hip_ops.knn_radius_update_raw(qd, qn, cd, cn, kth)
    _distances_close(kth.cpu().numpy(), ans['radius'])
    # the candidates' radii among the queries (the transposed search), then membership of the queries in those balls
    ckth = hip_ops.knn_radius_state(nc, 4, cuda_device)
    hip_ops.knn_radius_update_raw(cd, cn, qd, qn, ckth)
    _distances_close(ckth[:, :3].cpu().numpy(), ans['cand_radius'])
    member = torch.zeros((nq, 3), device=cuda_device, dtype=torch.int32)
    hip_ops.manifold_member_update_raw(qd, qn, cd, cn, ckth[:, :3].contiguous(), member)
    print('members per column %s of %d' % (ans['member'].sum(axis=0).tolist(), nq))
    assert np.array_equal(member.cpu().numpy() != 0, ans['member'])


@pytest.mark.parametrize('family', FLAT_LIKE)
def test_dci_rerank_path_on_adversarial_rows(cuda_device, family):
    """k = 17 is past the streaming kernel's lists: DCI.query_device_k screens with torch ops on the same product and the same
    interval (its sufficiency check restates nn1_tol), then re-ranks in fp64."""
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.dci_code.dci import DCI
    k, dim = hip_ops.NNK_MAX_K + 1, 12288
    q, c, ans = S.cut(family, 72, 136, dim)
    assert not S.undecided(ans['d2'], q, c, k + 1)
    want = np.argsort(ans['d2'], axis=1, kind='stable')[:, :k]
    db = DCI(dim, device=cuda_device)
    db.add(_dev(c, cuda_device))
    idx, dist = db.query(_dev(q, cuda_device), num_neighbours=k)
    assert np.array_equal(np.stack(idx), want)
    _distances_close(np.stack(dist) ** 2, np.take_along_axis(ans['d2'], want, 1))


@pytest.mark.parametrize('shape,dim,family', KMEANS)
def test_kmeans_step_on_adversarial_rows(cuda_device, shape, dim, family):
    from inclusivegan_amd import hip_ops
    RTOL = 1e-11        # tests/test_gpu_prd.py
    q, c, ans, qd, cd, _ = _operands(cuda_device, shape, family, dim)
    assert c.shape[0] == 20          # the 20 centres of PRD, drawn from the candidates: brute()'s labels are among the first 20
    label, d2, sums, count, inertia = [o.cpu().numpy() for o in hip_ops.kmeans_step(qd, hip_ops.row_sqnorm_raw(qd), cd)]
    assert np.array_equal(label, ans['label'])
    assert np.array_equal(count, np.bincount(ans['label'], minlength=20))
    assert np.all(np.abs(d2 - ans['label_d2']) <= RTOL * ans['label_d2'])
    assert abs(float(inertia[0]) - ans['label_d2'].sum()) <= RTOL * ans['label_d2'].sum()
