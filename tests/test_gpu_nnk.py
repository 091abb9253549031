"""GPU: the streaming exact k-NN with indices (igan_nnk_update, csrc/exact_search.hip) against the fp64 brute force of tests/imle_cases.py,
through hip_ops, DCI.query and the exclusive branch of imle_refresh.  Indices must be equal; distances are held to the bar of
tests/test_gpu_ops.py::test_knn_k_neighbours_vs_oracle, <= 1e-12 * max: the rows are fp32 and both sides sum direct differences
in fp64, so they differ by the summation order alone (~sqrt(dim) * 2^-53 relative).

Shapes: 257 candidates fed as 100 + 100 + 57 (a ragged tail, no batch a multiple of the 64 lanes, two 256-thread blocks for the
40 queries), at dim 7 (scalar path of wave_sqdist), 64 and 768 (16-byte path, one and three strides), and k on both sides of
the compiled list lengths 4 / 8 / 16."""
import functools

import numpy as np
import pytest
import torch

from imle_cases import exact_knn

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
BATCHES = ((0, 100), (100, 200), (200, 257))
KS = (1, 2, 10, 16)


@functools.lru_cache(maxsize=None)
def _case(dim):
    """(data [257, dim], queries [40, dim]) with the planted ties, and the oracle at k = 16 (every smaller k is a prefix)."""
    rng = np.random.RandomState(100 + dim)
    data = rng.uniform(-1, 1, size=(257, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, size=(40, dim)).astype(np.float32)
    data[41] = q[0]; data[41, 5] += 0.25                                       # very close to query 0
    data[150] = data[41]                                                       # its exact duplicate, in a later batch
    data[230] = q[0]; data[230, 2] += np.float32(0.25 * (1 + 2.0 ** -12))      # a near-tie behind them, 2^-12 relative apart
    data[120] = q[1]; data[120, 4] += 0.25                                     # very close to query 1
    data[20] = data[120]                                                       # its exact duplicate, in an EARLIER batch
    oi, od = exact_knn(data, q, 16)
    return data, q, oi, od                  # shared by the tests: never written to


def _feed(dev, data, q, k, batches, update=None):
    from inclusivegan_amd import hip_ops
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    qn = hip_ops.row_sqnorm_raw(qd)
    if update is None:
        state, update = hip_ops.nnk_state(q.shape[0], k, dev), hip_ops.nnk_update_raw
    else:
        state = hip_ops.nn1_state(q.shape[0], dev)
    for b0, b1 in batches:
        c = torch.from_numpy(np.ascontiguousarray(data[b0:b1])).to(dev)
        update(qd, qn, c, hip_ops.row_sqnorm_raw(c), state[0], state[1], b0)
    return state


def _check(state, oi, od, k):
    d2, idx = state[0].cpu().numpy(), state[1].cpu().numpy()
    assert idx.dtype == np.int32 and d2.dtype == np.float64 and idx.shape == d2.shape == (oi.shape[0], k)
    assert np.array_equal(idx, oi[:, :k])
    err = np.abs(np.sqrt(d2) - od[:, :k]).max()
    print('k %d: largest distance error %.3e, bar %.3e' % (k, err, 1e-12 * od.max()))
    assert err <= 1e-12 * od.max()


@pytest.mark.parametrize('dim', [7, 64, 3 * 16 * 16])
def test_against_the_oracle_in_any_order(cuda_device, dim):
    data, q, oi, od = _case(dim)
    for k in KS:
        fwd = _feed(cuda_device, data, q, k, BATCHES)
        _check(fwd, oi, od, k)
        # the state is a function of the set of (row, index) pairs fed: bits included
        for other in (BATCHES[::-1], ((0, 257),)):
            got = _feed(cuda_device, data, q, k, other)
            assert torch.equal(got[0], fwd[0]) and torch.equal(got[1], fwd[1]), (k, other)


@pytest.mark.parametrize('dim', [7, 64, 3 * 16 * 16])
def test_k1_is_the_1nn_state_bit_for_bit(cuda_device, dim):
    from inclusivegan_amd import hip_ops
    data, q, oi, od = _case(dim)
    for batches in (BATCHES, BATCHES[::-1]):
        d2, idx = _feed(cuda_device, data, q, 1, batches)
        bd, bi = _feed(cuda_device, data, q, 1, batches, update=hip_ops.nn1_update_raw)
        assert torch.equal(d2[:, 0], bd) and torch.equal(idx[:, 0], bi)


def test_ties_go_to_the_lower_index_both_ways(cuda_device):
    """Query 0: row 150 (a later batch) duplicates row 41 exactly.  Fed forwards the duplicate arrives later with the higher index and
    must queue behind; fed backwards row 41 arrives later, ties the distance and must displace -- at k = 1 and k = 2 it ties the
    k-th pair itself.  Row 230 is 2^-12 relative behind them: the exact order holds.  Query 1: row 20 (an earlier batch) duplicates
    row 120; with the middle batch fed first, row 20 arrives later and must come first."""
    data, q, oi, od = _case(3 * 16 * 16)
    assert list(oi[0, :3]) == [41, 150, 230] and od[0, 0] == od[0, 1] < od[0, 2]
    assert list(oi[1, :2]) == [20, 120] and od[1, 0] == od[1, 1] < od[1, 2]
    for k in (1, 2, 3, 10):
        for batches in (BATCHES, BATCHES[::-1], (BATCHES[1], BATCHES[0], BATCHES[2])):
            d2, idx = _feed(cuda_device, data, q[:2], k, batches)
            assert idx.cpu().numpy().tolist() == oi[:2, :k].tolist(), (k, batches)
            if k >= 3:
                assert float(d2[0, 0]) == float(d2[0, 1]) < float(d2[0, 2])
                assert float(d2[1, 0]) == float(d2[1, 1]) < float(d2[1, 2])


def test_small_sets_leave_the_trailing_slots_untouched(cuda_device):
    data, q, _, _ = _case(64)
    k = 10
    # batches smaller than k, and a whole stream of 5 < k candidates
    d2, idx = _feed(cuda_device, data, q, k, ((0, 3), (3, 5)))
    oi, od = exact_knn(data[:5], q, 5)
    assert np.array_equal(idx[:, :5].cpu().numpy(), oi)
    assert np.abs(np.sqrt(d2[:, :5].cpu().numpy()) - od).max() <= 1e-12 * od.max()
    assert bool(torch.isposinf(d2[:, 5:]).all()) and bool((idx[:, 5:] == INT32_MAX).all())
    # small batches that do fill the lists
    small = tuple((b, min(b + 7, 40)) for b in range(0, 40, 7))
    oi, od = exact_knn(data[:40], q, k)
    _check(_feed(cuda_device, data, q, k, small), oi, od, k)


def test_non_finite_rows_never_enter(cuda_device):
    data, q, _, _ = _case(64)
    data = data.copy()
    data[5, 3] = np.nan
    data[120, 0] = np.inf
    finite = np.asarray([i for i in range(257) if i not in (5, 120)])
    for k in (1, 10):
        oi, od = exact_knn(data[finite], q, k)
        _check(_feed(cuda_device, data, q, k, BATCHES), finite[oi].astype(np.int32), od, k)
    # nothing but non-finite rows: the state stays as initialised
    d2, idx = _feed(cuda_device, data, q, 3, ((5, 6), (120, 121)))
    assert bool(torch.isposinf(d2).all()) and bool((idx == INT32_MAX).all())


def test_dci_query_runs_on_the_streaming_kernel(cuda_device, monkeypatch):
    from inclusivegan_amd.dci_code.dci import DCI
    rng = np.random.RandomState(3)
    data = rng.uniform(-1, 1, size=(700, 3 * 16 * 16)).astype(np.float32)
    q = rng.uniform(-1, 1, size=(33, data.shape[1])).astype(np.float32)
    db = DCI(data.shape[1], 3, 15, device=cuda_device)
    db.cand_chunk = 256
    db.add(torch.from_numpy(data).to(cuda_device))
    qd = torch.from_numpy(q).to(cuda_device)
    want_i, want_d = db.query_device_k(qd, 10)
    with monkeypatch.context() as m:
        m.setattr(DCI, 'query_device_k', lambda *a, **kw: pytest.fail('k = 10 went to query_device_k'))
        idx, dist = db.query(qd, num_neighbours=10)
    assert idx[0].dtype == np.int32 and dist[0].dtype == np.float64
    assert np.array_equal(np.stack(idx), want_i.cpu().numpy())
    assert np.abs(np.stack(dist) - want_d.cpu().numpy()).max() <= 1e-12 * float(want_d.max())
    # beyond NNK_MAX_K the torch re-rank still answers
    with monkeypatch.context() as m:
        m.setattr(DCI, 'query_device_nnk', lambda *a, **kw: pytest.fail('k = 17 went to the streaming kernel'))
        idx, dist = db.query(qd, num_neighbours=17)
    oi, od = exact_knn(data, q, 17)
    assert np.array_equal(np.stack(idx), oi)
    assert np.abs(np.stack(dist) - od).max() <= 1e-12 * od.max()


# ----------------------------------------------------------------------------- the exclusive refresh
class _Rec:
    """A `training_set_rec` stand-in: uint8 images served in data-set order, 2 * minibatch per pull."""

    def __init__(self, images):
        self.images = images
        self.shape = list(images.shape[1:])
        self.dynamic_range = [0, 255]
        self.cur = 0

    def get_minibatch_np(self, n):
        out = self.images[self.cur:self.cur + n]
        self.cur = (self.cur + n) % self.images.shape[0]
        return out, np.zeros((n, 0), np.float32)


class _G:
    """get_output_for(latents, labels, is_validation=True) -> [n, 3, R, R] images in [-1, 1]: tanh of a fixed linear map."""

    def __init__(self, res, device, seed):
        g = torch.Generator().manual_seed(seed)
        self.w = (torch.randn(16, 3 * res * res, generator=g) * 0.5).to(device)
        self.res = res

    def get_output_for(self, z, lab, is_validation=False):
        return torch.tanh(z @ self.w).reshape(z.shape[0], 3, self.res, self.res).contiguous(memory_format=torch.channels_last)


def _refresh_fixture(dev):
    res, data_size, factor, mb = 8, 24, 5, 3
    rng = np.random.RandomState(11)
    images = rng.randint(0, 256, size=(data_size, 3, res, res)).astype(np.uint8)
    lat = rng.randn(data_size * factor, 16).astype(np.float32)
    labels = np.zeros((data_size * factor, 0), np.float32)
    return images, _G(res, dev, 5), lat, labels, data_size, mb


def _raise(*a, **kw):
    raise AssertionError('the exclusive refresh went to DCI.query_device_k')


def test_exclusive_refresh_streams(cuda_device, monkeypatch):
    from inclusivegan_amd.dci_code.dci import DCI
    from inclusivegan_amd.training import training_loop as TL
    from inclusivegan_amd.training import misc
    images, G, lat, labels, data_size, mb = _refresh_fixture(cuda_device)
    k = 3
    assert TL.NNK_STREAM is True
    with monkeypatch.context() as m:
        m.setattr(DCI, 'query_device_k', _raise)
        rec = _Rec(images)
        idx, dist = TL.imle_refresh(G, rec, lat, labels, data_size, mb, 32, [-1, 1], cuda_device, exclusive_k=k, cand_pack=32)
        assert rec.cur == 0
    with torch.no_grad():
        cands = G.get_output_for(torch.from_numpy(lat).to(cuda_device), None).contiguous().reshape(lat.shape[0], -1).cpu().numpy()
    reals = misc.adjust_dynamic_range(images.astype(np.float32), [0, 255], [-1, 1]).reshape(data_size, -1)
    oi, od = exact_knn(cands, reals, k)
    want_i, want_d = TL.exclusive_assignment(oi, od)
    assert idx.shape == (data_size,) and dist.dtype == np.float64
    assert np.array_equal(idx, want_i)
    # the reals are range-adjusted in fp32 on the device and on the host (one rounding each): tests/test_gpu_refresh.py's bar
    assert np.allclose(dist, want_d, rtol=1e-6, atol=0)
    # the resident path (IGAN_NNK_STREAM=0) on the same inputs: the same rows on both sides, only the summation order differs
    with monkeypatch.context() as m:
        m.setattr(TL, 'NNK_STREAM', False)
        m.setattr(TL.hip_ops, 'nnk_update_raw', lambda *a, **kw: pytest.fail('IGAN_NNK_STREAM=0 still streams'))
        idx0, dist0 = TL.imle_refresh(G, _Rec(images), lat, labels, data_size, mb, 32, [-1, 1], cuda_device, exclusive_k=k, cand_pack=32)
    assert np.array_equal(idx, idx0)
    assert np.abs(dist - dist0).max() <= 1e-12 * dist0.max()


def test_rank_shards_merge_to_the_single_rank_lists(cuda_device, monkeypatch):
    """Ranks 0 and 1 of a world of 2, replayed one after the other up to their k-NN lists, merged by the module's own merge: the
    world-1 lists, indices and bits.  A world of 8 leaves ranks 4 .. 7 without a pack: they contribute the untouched state."""
    from inclusivegan_amd.dci_code.dci import DCI
    from inclusivegan_amd.training import training_loop as TL
    images, G, lat, labels, data_size, mb = _refresh_fixture(cuda_device)
    k = 3
    monkeypatch.setattr(DCI, 'query_device_k', _raise)

    def lists(rank, world):
        return TL.imle_search(G, _Rec(images), lat, labels, data_size, mb, 32, [-1, 1], cuda_device, rank=rank, world=world,
                              exclusive_k=k, cand_pack=32)

    one_i, one_d = lists(0, 1)
    assert one_i.dtype == torch.int64 and one_d.dtype == torch.float64 and one_i.shape == one_d.shape == (data_size, k)
    assert int(one_i.max()) < lat.shape[0] and bool(torch.isfinite(one_d).all())
    for world in (2, 8):
        parts = [lists(r, world) for r in range(world)]
        if world == 8:          # 120 candidates in packs of 32: four packs
            for gi, ld in parts[4:]:
                assert bool((gi == INT32_MAX).all()) and bool(torch.isposinf(ld).all())
        gi, ld = TL.merge_knn_lists([p[0] for p in parts], [p[1] for p in parts], k)
        assert torch.equal(gi, one_i) and torch.equal(ld, one_d), world
