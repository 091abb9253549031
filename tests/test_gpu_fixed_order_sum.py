"""GPU: the loop bounds of the shared folds of csrc/fixed_order_sum.h, per output element, through the raw wrappers
scale_dot_raw, bias_act_noise_bwd_raw (linear, gain 1, with and without noise), bias_act_noise_bwd_dd_raw (N = 2: the per-sample
block ranges) and bias_grad_raw.

Cases.  The number of per-block partials P that the column fold adds is chosen through the row count: a block takes
`unit` = 8 * rl rows (rl = 256 / min(C / 4, 256) row lanes), rows = P * unit + unit // 3, and every test reads the count back
from the library's workspace-size query and asserts it is P, so a change of the heuristic cannot empty the test.
P in {1, 15, 16, 17, 48, 49, 64, 65, 113} at C = 64 (one group; the last full round of 16; one past it; the four-accumulator
round of 64 less one, exact, and one past; a second round with a remainder); at P in {1, 17} also C = 4 (rl = 256), 12 (three
columns, one idle thread), 1028 (a second block of float4 columns); at C = 64 the column count C + 1 of the bias_act_noise
final kernel spills into a block of its own.  bias_grad_raw: rows layout with ceil(outer / 256) in {1, 3, 4, 5, 9} chunks and
size_b = 300, plane layout with step_b in {7, 64, 300}.

Inputs are drawn from [0.5, 1.5): every term is positive, so a lost or doubled partial moves its element by its whole share.
Assertion, per output ELEMENT: |got - fp64 sum| <= n * 2^-24 * sum |terms|, n the number of terms of the element and the terms
formed in fp64 from the float32 inputs -- the first-order bound of ANY summation order of n rounded terms, derived, not
measured.  (The dd case runs without bias, with strength 0 and with d in {0.5, 1, 2}: its terms are then the plain products
dy * y and the division is exact, as the bound assumes.)
For every case the CPU side confirms that the test is sharp: the smallest partial of any element is at least 3 bounds large.
Two outputs cannot meet that with this bound, whatever the rows: dstrength has n = rows * C terms, and db of the dd op sums the
2 P blocks of both samples (at P = 113, 226 blocks of >= 128 rows: the smallest partial is 1.1 bounds).  Next to the bound above
these two are held to k * 2^-24 * sum |terms|, k the longest chain of roundings a term meets in the kernels' order --
ceil(rows per block / rl) additions in the thread, then for dstrength 4 (the product with a float4's sum) and 8 (block sum),
for db rl (row-lane fold), then ceil(blocks / 16) + 2 in a group of the column fold and 16 over its groups -- and their
sharpness is confirmed against that.
The same call made twice returns the same bytes, every output of every case.
Measured on the MI355X (each figure is printed before it is asserted): worst |err| / bound 0.31, worst |err| / chain bound
0.11, smallest partial 3.98 bounds (dot, C = 64, P = 113)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CASES = [(64, p) for p in (1, 15, 16, 17, 48, 49, 64, 65, 113)] + [(c, p) for c in (4, 12, 1028) for p in (1, 17)]
IDS = ['C%d-P%d' % cp for cp in CASES]


def row_lanes(C):
    return 256 // min(C // 4, 256)


def rows_for(C, P):
    unit = 8 * row_lanes(C)
    return P * unit + unit // 3


def block_ranges(rows, P, base=0):
    """[start, end) of the rows each of P blocks sums (ceil(rows / P) rows per block, the last one short)."""
    per = -(-rows // P)
    return [(base + j * per, base + min((j + 1) * per, rows)) for j in range(P)]


def rand(gen, *shape):
    return torch.rand(*shape, generator=gen, dtype=torch.float32) + 0.5


def check(name, got, terms, axes, ranges, chain=None):
    """terms: fp64 array whose sum over `axes` is the expected output; axis 0 is the one the blocks cut into `ranges`.
    Asserts the bound per element, then that the smallest partial of any element is >= 3 bounds (against the chain bound where
    one is given: see the module docstring)."""
    got = np.asarray(got, dtype=np.float64)
    ref = terms.sum(axis=axes)
    mag = np.abs(terms).sum(axis=axes)
    n = int(np.prod([terms.shape[a] for a in np.atleast_1d(axes)]))
    bound = n * U * mag
    err = np.abs(got.reshape(ref.shape) - ref)
    print('%-22s n %8d  worst |err| / bound %.3g' % (name, n, float((err / bound).max())))
    assert (err <= bound).all(), name
    sharp = bound
    if chain is not None:
        sharp = chain * U * mag
        print('%-22s chain %d  worst |err| / chain bound %.3g' % (name, chain, float((err / sharp).max())))
        assert (err <= sharp).all(), name + ' (chain bound)'
    smallest = np.min([terms[a:b].sum(axis=axes) for a, b in ranges if b > a], axis=0)
    print('%-22s smallest partial / bound %.3g' % (name, float((smallest / sharp).min())))
    assert (smallest >= 3.0 * sharp).all(), name + ': the bound would hide a lost partial'


def same_bytes(a, b):
    for x, y in zip(a, b):
        if x is None:
            assert y is None
        else:
            assert torch.equal(x, y) and x.dtype == y.dtype


def column_fold_chain(P):
    return -(-P // 16) + 2 + 16


def ds_chain(rows_per_block, C, P):
    return 4 + -(-rows_per_block // row_lanes(C)) + 8 + column_fold_chain(P)


def db_chain(rows_per_block, C, P):
    return -(-rows_per_block // row_lanes(C)) + row_lanes(C) + column_fold_chain(P)


@pytest.mark.parametrize('C,P', CASES, ids=IDS)
def test_scale_dot(cuda_device, C, P):
    from inclusivegan_amd import _abi, hip_ops
    N, HW = 2, rows_for(C, P)
    assert int(_abi.get_plugin().igan_scale_dot_workspace_floats(N, HW, C)) == N * P * C
    gen = torch.Generator().manual_seed(C * 1000 + P)
    a, b = rand(gen, N, HW, 1, C), rand(gen, N, HW, 1, C)
    run = lambda: hip_ops.scale_dot_raw(a.to(cuda_device).permute(0, 3, 1, 2), b.to(cuda_device).permute(0, 3, 1, 2))
    first, again = run(), run()
    same_bytes(first, again)
    terms = (a.double() * b.double()).numpy().reshape(N, HW, C)
    for n in range(N):
        check('dot[%d]' % n, first[0][n].cpu().numpy(), terms[n], 0, block_ranges(HW, P))


@pytest.mark.parametrize('C,P', CASES, ids=IDS)
def test_bias_act_noise_bwd(cuda_device, C, P):
    from inclusivegan_amd import _abi, hip_ops
    rows = rows_for(C, P)
    assert int(_abi.get_plugin().igan_bias_act_noise_workspace_floats(rows, C)) == P * (C + 1)
    gen = torch.Generator().manual_seed(C * 1000 + P + 1)
    dy, y, nz = rand(gen, rows, C), rand(gen, rows, C), rand(gen, rows)
    ranges = block_ranges(rows, P)
    for noise in (None, nz):
        run = lambda: hip_ops.bias_act_noise_bwd_raw(dy.to(cuda_device), y.to(cuda_device), None if noise is None else noise.to(cuda_device), 1, 0.0, 1.0, True)
        if noise is not None and C > 1024:
            # only the first block of 256 float4 columns adds its noise-strength sums: the op must refuse, not drop the rest
            with pytest.raises(ValueError, match='C must be <= 1024'):
                run()
            continue
        first, again = run(), run()
        same_bytes(first, again)
        dx, db, ds = first
        assert torch.equal(dx.cpu(), dy)                       # linear, gain 1
        check('db', db.cpu().numpy(), dy.double().numpy(), 0, ranges)
        if noise is None:
            assert ds is None
        else:
            check('dstrength', ds.cpu().numpy(), (nz.double()[:, None] * dy.double()).numpy(), (0, 1), ranges,
                  chain=ds_chain(ranges[0][1] - ranges[0][0], C, P))


@pytest.mark.parametrize('C,P', CASES, ids=IDS)
def test_bias_act_noise_bwd_dd(cuda_device, C, P):
    from inclusivegan_amd import _abi, hip_ops
    N, HW = 2, rows_for(C, P)
    assert int(_abi.get_plugin().igan_bias_act_noise_dd_workspace_floats(N, HW, C)) == N * P * (2 * C + 1)
    gen = torch.Generator().manual_seed(C * 1000 + P + 2)
    dy, y = rand(gen, N, HW, 1, C), rand(gen, N, HW, 1, C)
    d = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N, C), generator=gen)]
    with_noise = C <= 1024                                     # the op takes noise up to C = 1024
    nz = rand(gen, N, 1, HW, 1) if with_noise else None
    to = lambda t: None if t is None else t.to(cuda_device)
    strength = torch.zeros(()) if with_noise else None
    run = lambda: hip_ops.bias_act_noise_bwd_dd_raw(to(dy).permute(0, 3, 1, 2), to(y).permute(0, 3, 1, 2), to(nz), to(strength), None, to(d), 1, 0.0, 1.0)
    first, again = run(), run()
    same_bytes(first, again)
    dx, db, ds, dd = first
    assert torch.equal(dx.permute(0, 2, 3, 1).cpu(), dy)
    g = dy.double().numpy().reshape(N * HW, C)
    ranges = [r for n in range(N) for r in block_ranges(HW, P, n * HW)]
    check('db', db.cpu().numpy(), g, 0, ranges, chain=db_chain(ranges[0][1] - ranges[0][0], C, 2 * P))
    prod = (dy.double() * y.double()).numpy().reshape(N, HW, C)
    for n in range(N):
        check('dd[%d]' % n, dd[n].cpu().numpy(), prod[n] / d[n].double().numpy(), 0, block_ranges(HW, P))
    if with_noise:
        check('dstrength', ds.cpu().numpy(), nz.double().numpy().reshape(N * HW, 1) * g, (0, 1), ranges,
              chain=ds_chain(ranges[0][1] - ranges[0][0], C, 2 * P))
    else:
        assert ds is None


@pytest.mark.parametrize('chunks', [1, 3, 4, 5, 9])
def test_bias_grad_rows(cuda_device, chunks):
    from inclusivegan_amd import _abi, hip_ops
    outer, size_b = 256 * chunks - 19, 300
    assert int(_abi.get_plugin().igan_bias_grad_workspace_floats(outer * size_b, size_b, 1)) == chunks * size_b
    dx = rand(torch.Generator().manual_seed(chunks), outer, size_b)
    run = lambda: hip_ops.bias_grad_raw(dx.to(cuda_device), size_b, 1)
    first, again = run(), run()
    same_bytes([first], [again])
    check('db', first.cpu().numpy(), dx.double().numpy(), 0, [(256 * j, min(256 * (j + 1), outer)) for j in range(chunks)])


@pytest.mark.parametrize('step_b', [7, 64, 300])
def test_bias_grad_planes(cuda_device, step_b):
    from inclusivegan_amd import _abi, hip_ops
    outer, size_b = 5, 6
    assert int(_abi.get_plugin().igan_bias_grad_workspace_floats(outer * size_b * step_b, size_b, step_b)) == outer * size_b
    dx = rand(torch.Generator().manual_seed(step_b), outer, size_b, step_b)
    run = lambda: hip_ops.bias_grad_raw(dx.to(cuda_device), size_b, step_b)
    first, again = run(), run()
    same_bytes([first], [again])
    check('db', first.cpu().numpy(), dx.double().numpy(), (0, 2), [(o, o + 1) for o in range(outer)])
