"""GPU: the one place where the exact searches of csrc/exact_search.hip differ on purpose, pinned -- what a NaN screening value
decides (csrc/exact_search.h: contends_if_decided / contends_unless_ruled_out; include/igan_hip.h, igan_nnk_update).

3 queries x 70 candidates (one full strip of 64 lanes and a ragged tail of 6) of uniform values, at dim 36 (the 16-byte path of
wave_sqdist) and dim 35 (the scalar path).  Query 0 and candidate 66 are flat rows of 1e20: their squared norms (dim * 1e40)
round to +inf in fp32 and so does their fp32 product, so |q|^2 + |c|^2 - 2 q.c is inf + inf - inf = NaN for that pair, and
a = +inf, a - t = NaN for every pair with one of the two rows.  The fp64 direct difference of the two flat rows is exactly 0.
  igan_nn1_update   drops a candidate the interval cannot decide: query 0 measures nothing and stays (+inf, INT32_MAX);
  igan_nnk_update   measures it: with k = 1 query 0 gets (0.0, 66).
Queries 1 and 2 are ordinary rows: the two entries agree there, and with the fp64 brute force (candidate 66 lies ~1e20 away).
The parent of the commit that introduced this file (the five hand-written kernels) gives the same values: the test pins them."""
import functools

import numpy as np
import pytest
import torch

from imle_cases import exact_knn

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
NQ, NC, FLAT = 3, 70, 66


@functools.lru_cache(maxsize=None)
def _case(dim):
    rng = np.random.RandomState(7 + dim)
    q = rng.uniform(-1, 1, size=(NQ, dim)).astype(np.float32)
    c = rng.uniform(-1, 1, size=(NC, dim)).astype(np.float32)
    q[0] = 1e20
    c[FLAT] = 1e20
    oi, od = exact_knn(c, q, 1)
    return q, c, oi[:, 0], od[:, 0]         # shared: never written to


@pytest.mark.parametrize('dim', [36, 35])
def test_nan_screening_value_is_dropped_by_nn1_and_measured_by_nnk(dim):
    from inclusivegan_amd import hip_ops
    dev = torch.device('cuda')
    q, c, oi, od = _case(dim)
    assert oi[0] == FLAT and od[0] == 0.0                              # the brute force: the flat pair is at distance exactly 0
    qd, cd = torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev)
    qn, cn = hip_ops.row_sqnorm_raw(qd), hip_ops.row_sqnorm_raw(cd)
    assert bool(torch.isposinf(qn[0])) and bool(torch.isposinf(cn[FLAT]))
    d1, i1 = hip_ops.nn1_state(NQ, dev)
    hip_ops.nn1_update_raw(qd, qn, cd, cn, d1, i1, 0)
    dk, ik = hip_ops.nnk_state(NQ, 1, dev)
    hip_ops.nnk_update_raw(qd, qn, cd, cn, dk, ik, 0)
    d1, i1, dk, ik = d1.cpu().numpy(), i1.cpu().numpy(), dk.cpu().numpy()[:, 0], ik.cpu().numpy()[:, 0]
    print('dim %d: nn1 %s %s   nnk(k=1) %s %s   brute force %s %s' % (dim, d1, i1, dk, ik, od ** 2, oi))
    assert np.isposinf(d1[0]) and i1[0] == INT32_MAX                   # 1-NN: undecidable, never measured
    assert dk[0] == 0.0 and ik[0] == FLAT                              # k lists: measured, enters on its fp64 distance
    assert np.array_equal(i1[1:], oi[1:]) and np.array_equal(ik[1:], oi[1:])
    assert np.array_equal(d1[1:], dk[1:])                              # one wave_sqdist: the same bits
    err = np.abs(np.sqrt(d1[1:]) - od[1:]).max()
    print('         largest distance error on the ordinary queries %.3e, bar %.3e' % (err, 1e-12 * od[1:].max()))
    assert err <= 1e-12 * od[1:].max()                                 # the bar of tests/test_gpu_nnk.py: summation order alone


def test_nn1_update_checks_shapes():
    """nn1_update_raw shares the operand check of the other three wrappers: norms that do not match their rows are refused."""
    from inclusivegan_amd import hip_ops
    dev = torch.device('cuda')
    q, c = torch.zeros(8, 4, device=dev), torch.zeros(6, 4, device=dev)
    d2, idx = hip_ops.nn1_state(8, dev)
    with pytest.raises(ValueError):
        hip_ops.nn1_update_raw(q, torch.zeros(8, device=dev), c, torch.zeros(5, device=dev), d2, idx, 0)
    with pytest.raises(ValueError):
        hip_ops.nn1_update_raw(q, torch.zeros(8, device=dev), torch.zeros(6, 5, device=dev), torch.zeros(6, device=dev), d2, idx, 0)
    with pytest.raises(ValueError):
        hip_ops.nn1_update_raw(q, torch.zeros(8, device=dev), c, torch.zeros(6, device=dev), d2[:7], idx[:7], 0)
