"""GPU: igan_manifold_member_nn1_update -- membership and nearest neighbour of a candidate batch on one product block.

Contract: member, best_d2 and best_idx end, bit for bit, as igan_manifold_member_update followed by igan_nn1_update on the
same arguments leave them.  nq = 70, nc = 130 (two full 64-candidate strips and a tail of 2), dim = 67, nk = 2, the candidates
fed in three batches of 50 / 50 / 30 with their idx_base.  Every case is compared (tobytes) with the two existing entries run
on fresh copies of the same states, and with the fp64 brute force of tests/test_precision_recall.py: membership and nearest
index exactly, the nearest distance within (dim + 2) 2^-52 relative -- both sides sum dim exact fp64 squares of exact
differences, in different orders, and an fp64 sum of dim non-negative terms is within (dim - 1) 2^-53 relative of the true
sum whatever the order."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_precision_recall import brute_evaluate, brute_manifold, brute_sqdist  # noqa: E402

pytestmark = pytest.mark.gpu

NQ, NC, DIM, NK = 70, 130, 67, 2
BATCHES = ((0, 50), (50, 100), (100, 130))
INT32_MAX = 2 ** 31 - 1


def base_rows(seed):
    """Queries and candidates; the first 35 queries sit next to a candidate, so the memberships are mixed."""
    rng = np.random.RandomState(seed)
    c = rng.randn(NC, DIM).astype(np.float32)
    q = rng.randn(NQ, DIM).astype(np.float32)
    near = rng.randint(0, NC, size=35)
    q[:35] = c[near] + 0.3 * rng.randn(35, DIM).astype(np.float32)
    return q, c


def feed(dev, q, c, radii, one_product, member0=None):
    """The three batches through the new entry, or through the two existing ones -> (member, best_d2, best_idx) on the host."""
    from inclusivegan_amd import hip_ops
    qd, cd = torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev)
    rad = torch.from_numpy(np.ascontiguousarray(radii, np.float64)).to(dev)
    qn = hip_ops.row_sqnorm_raw(qd)
    member = torch.zeros((NQ, NK), device=dev, dtype=torch.int32) if member0 is None else torch.from_numpy(member0).to(dev)
    d2, idx = hip_ops.nn1_state(NQ, dev)
    for b, e in BATCHES:
        cb = cd[b:e]
        cn = hip_ops.row_sqnorm_raw(cb)
        if one_product:
            hip_ops.manifold_member_nn1_update_raw(qd, qn, cb, cn, rad[b:e], member, d2, idx, b)
        else:
            hip_ops.manifold_member_update_raw(qd, qn, cb, cn, rad[b:e], member)
            hip_ops.nn1_update_raw(qd, qn, cb, cn, d2, idx, b)
    torch.cuda.synchronize()
    return member.cpu().numpy(), d2.cpu().numpy(), idx.cpu().numpy()


def check(dev, q, c, radii, member0=None, brute_rows=None):
    """New entry == the pair of entries, bit for bit; both == the brute force on `brute_rows` (default: all queries)."""
    got = feed(dev, q, c, radii, True, member0)
    pair = feed(dev, q, c, radii, False, member0)
    for what, a, b in zip(('member', 'best_d2', 'best_idx'), got, pair):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
    member, d2, idx = got
    rows = np.arange(NQ) if brute_rows is None else np.asarray(brute_rows)
    pred, _, nearest = brute_evaluate(c, np.asarray(radii, np.float64), q)
    if member0 is not None:
        pred = pred | (member0 != 0)
    dmin = brute_sqdist(q, c).min(axis=1)
    assert np.array_equal(member[rows], pred[rows])
    assert np.array_equal(idx[rows], nearest[rows])
    assert np.all(np.abs(d2[rows] - dmin[rows]) <= (DIM + 2) * 2.0 ** -52 * dmin[rows])
    return got


def test_random_rows(cuda_device):
    q, c = base_rows(1)
    radii = brute_manifold(c, [2, 4])
    member, _, _ = check(cuda_device, q, c, radii)
    assert 0 < member.sum() < member.size            # the case decides something


def test_every_query_a_member_after_the_first_batch(cuda_device):
    """Radii of 1e30 in batch 1 set every column of every query there; each query's nearest candidate arrives in batch 3.
    A fold that left with the membership walk would miss it."""
    rng = np.random.RandomState(2)
    q, c = base_rows(2)
    home = 100 + np.arange(NQ) % 30
    q = (c[home] + 1e-3 * rng.randn(NQ, DIM)).astype(np.float32)
    radii = brute_manifold(c, [2, 4])
    radii[:50] = 1e30
    member, d2, idx = check(cuda_device, q, c, radii)
    assert member.all()
    assert np.array_equal(idx, home.astype(np.int32)) and np.all(d2 < 1e-3)
    # and the state after batch 1 alone was already all ones: the early exit is taken in batches 2 and 3
    after1 = brute_evaluate(c[:50], radii[:50], q)[0]
    assert after1.all()


def test_duplicated_candidates_go_to_the_lower_index(cuda_device):
    rng = np.random.RandomState(3)
    q, c = base_rows(3)
    c[97] = c[3]
    q[:10] = (c[3] + 0.05 * rng.randn(10, DIM)).astype(np.float32)
    q[10] = c[3]                                       # an exact copy: distance 0
    _, d2, idx = check(cuda_device, q, c, brute_manifold(c, [2, 4]))
    assert np.all(idx[:11] == 3) and d2[10] == 0.0


def test_nan_query_row(cuda_device):
    q, c = base_rows(4)
    q[5] = np.nan
    q[44, 9] = np.nan
    keep = np.setdiff1d(np.arange(NQ), [5, 44])
    member, d2, idx = check(cuda_device, q, c, brute_manifold(c, [2, 4]), brute_rows=keep)
    for r in (5, 44):
        assert not member[r].any() and idx[r] == INT32_MAX and d2[r] == np.inf


def test_candidate_row_whose_norm_overflows_fp32(cuda_device):
    """Row 7 = 1e20: |c|^2 is +inf in fp32 and the screening value of every pair with it is not a number.  The 1-NN half drops
    such a candidate, the membership half measures it: its exact distance, 6.7e41, is finite and within its radius of 1e300 in
    column 0, and outside its radius of 0 in column 1."""
    q, c = base_rows(5)
    c[7] = 1e20
    radii = brute_manifold(c, [2, 4])
    radii[7] = (1e300, 0.0)
    member, _, idx = check(cuda_device, q, c, radii)
    assert member[:, 0].all() and not member[:, 1].all() and not (idx == 7).any()


def test_member_all_ones_on_entry(cuda_device):
    q, c = base_rows(6)
    ones = np.ones((NQ, NK), np.int32)
    member, d2, idx = check(cuda_device, q, c, brute_manifold(c, [2, 4]), member0=ones)
    assert member.all() and np.all(idx < NC) and np.all(np.isfinite(d2))


def test_same_bits_twice(cuda_device):
    q, c = base_rows(1)
    radii = brute_manifold(c, [2, 4])
    first = feed(cuda_device, q, c, radii, True)
    again = feed(cuda_device, q, c, radii, True)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


def test_wrapper_checks_its_operands(cuda_device):
    from inclusivegan_amd import hip_ops
    dev = cuda_device
    q, c = torch.zeros(8, 5, device=dev), torch.zeros(6, 5, device=dev)
    qn, cn = torch.zeros(8, device=dev), torch.zeros(6, device=dev)
    rad = torch.zeros(6, 2, device=dev, dtype=torch.float64)
    member = torch.zeros(8, 2, device=dev, dtype=torch.int32)
    d2, idx = hip_ops.nn1_state(8, dev)
    with pytest.raises(ValueError):
        hip_ops.manifold_member_nn1_update_raw(q, qn, c, cn[:5], rad, member, d2, idx, 0)
    with pytest.raises(ValueError):
        hip_ops.manifold_member_nn1_update_raw(q, qn, c, cn, rad[:5], member, d2, idx, 0)
    with pytest.raises(ValueError):
        hip_ops.manifold_member_nn1_update_raw(q, qn, c, cn, rad, member, d2[:7], idx[:7], 0)
    with pytest.raises(TypeError):
        hip_ops.manifold_member_nn1_update_raw(q, qn, c, cn, rad.float(), member, d2, idx, 0)
    with pytest.raises(TypeError):
        hip_ops.manifold_member_nn1_update_raw(q, qn, c, cn, rad, member, d2.float(), idx, 0)
    with pytest.raises(ValueError, match='overflows int32'):
        hip_ops.manifold_member_nn1_update_raw(q, qn, c, cn, rad, member, d2, idx, INT32_MAX - 3)
