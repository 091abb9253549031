"""GPU: the exact manifold search over row shards, replayed in one process.

Every state of the search is a function of the set of (row, index) pairs fed to it, so a search over rows [b, e) against
all columns gives exactly the rows [b, e) of the whole search.  The row-range forms of the two passes
(ManifoldEstimator.radii_rows / evaluate_rows) are run for every rank of a world in turn, concatenated in rank order and
compared with the whole-set knn_precision_recall_features state: tobytes() for arrays, == for the two means.  One whole-set
state is computed per shape and shared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K, ROW_BATCH, COL_BATCH = 3, 64, 50


def make_features(n_ref, n_eval, F, seed):
    rng = np.random.RandomState(seed)
    ref = rng.randn(n_ref, F).astype(np.float32)
    ev = (rng.randn(n_eval, F) * 1.1).astype(np.float32)
    if n_ref > 150:     # three duplicated rows: inside a set, across the sets, inside the other set
        ref[101] = ref[17]
        ev[5] = ref[17]
        ev[141] = ev[40]
    return ref, ev


@pytest.fixture(scope='module')
def big(cuda_device):
    from inclusivegan_amd.metrics import precision_recall as PR
    ref, ev = make_features(203, 190, 24, 11)
    whole = PR.knn_precision_recall_features(torch.from_numpy(ref).to(cuda_device), torch.from_numpy(ev).to(cuda_device), nhood_sizes=[K],
                                             row_batch_size=ROW_BATCH, col_batch_size=COL_BATCH)
    return ref, ev, whole


class Launches:
    """Counts the calls of the search wrappers that an estimator makes."""
    NAMES = ('row_sqnorm_raw', 'knn_radius_update_raw', 'manifold_member_update_raw', 'manifold_member_nn1_update_raw', 'nn1_update_raw')

    def __init__(self, monkeypatch):
        from inclusivegan_amd import hip_ops
        self.count = 0
        for name in self.NAMES:
            monkeypatch.setattr(hip_ops, name, self._wrap(getattr(hip_ops, name)))

    def _wrap(self, fn):
        def counted(*a, **k):
            self.count += 1
            return fn(*a, **k)
        return counted


def replay(dev, ref, ev, world, launches=None):
    """The four passes, each as the row ranges of ranks 0 .. world - 1 concatenated -> the state knn_precision_recall_features
    builds.  The radii of a set are complete before its membership pass starts, as under a group."""
    from inclusivegan_amd import dnnlib
    from inclusivegan_amd.metrics import precision_recall as PR
    state = dnnlib.EasyDict()
    sets = dict(ref=torch.from_numpy(ref).to(dev), eval=torch.from_numpy(ev).to(dev))
    manifolds = {}
    for name, feats in sets.items():
        m = PR.ManifoldEstimator(None, feats, ROW_BATCH, COL_BATCH, [K])
        parts = []
        for r in range(world):
            b, e = PR.search_rows(feats.shape[0], r, world)
            before = launches.count if launches else 0
            part = m.radii_rows(b, e)
            if launches and e == b:
                assert launches.count == before              # an empty range launches nothing
            assert part.shape == (e - b, 1) and part.dtype == torch.float64
            parts.append(part)
        m.D = torch.cat(parts).cpu().numpy().astype(np.float64)
        manifolds[name] = m
    state.ref_manifold, state.eval_manifold = manifolds['ref'], manifolds['eval']

    def evaluate(m, feats, want_nn):
        parts = []
        for r in range(world):
            b, e = PR.search_rows(feats.shape[0], r, world)
            before = launches.count if launches else 0
            parts.append(m.evaluate_rows(feats, b, e, want_nn))
            if launches and e == b:
                assert launches.count == before
            assert parts[-1][0].shape == (e - b, 1)
        member, d2, idx = (torch.cat([p[i] for p in parts]) for i in range(3))
        return m.evaluation_results(member, d2, idx, return_realism=want_nn, return_neighbors=want_nn)

    state.precision, state.realism_scores, state.nearest_neighbors = evaluate(state.ref_manifold, sets['eval'], True)
    state.knn_precision = state.precision.mean(axis=0)
    state.recall = evaluate(state.eval_manifold, sets['ref'], False)
    state.knn_recall = state.recall.mean(axis=0)
    return state


def assert_same_state(got, whole):
    assert got.ref_manifold.D.tobytes() == whole.ref_manifold.D.tobytes()
    assert got.eval_manifold.D.tobytes() == whole.eval_manifold.D.tobytes()
    for name in ('precision', 'recall', 'realism_scores', 'nearest_neighbors'):
        a, b = got[name], whole[name]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert np.all(got.knn_precision == whole.knn_precision) and np.all(got.knn_recall == whole.knn_recall)


@pytest.mark.parametrize('world', [1, 2, 3, 7])
def test_row_shards_concatenate_to_the_whole_search(cuda_device, big, world):
    ref, ev, whole = big
    assert_same_state(replay(cuda_device, ref, ev, world), whole)
    # the case is not a trivial one: both means are strictly between 0 and 1, and the planted copy has distance 0
    assert 0 < whole.knn_precision[0] < 1 and 0 < whole.knn_recall[0] < 1
    assert np.isinf(whole.realism_scores[5]) and whole.nearest_neighbors[5] == 17


def test_ranks_without_rows_launch_nothing(cuda_device, monkeypatch):
    from inclusivegan_amd.metrics import precision_recall as PR
    ref, ev = make_features(6, 6, 24, 12)
    whole = PR.knn_precision_recall_features(torch.from_numpy(ref).to(cuda_device), torch.from_numpy(ev).to(cuda_device), nhood_sizes=[K],
                                             row_batch_size=ROW_BATCH, col_batch_size=COL_BATCH)
    assert [PR.search_rows(6, r, 7) for r in range(7)].count((0, 0)) == 1     # rank 0 of 7 owns no row of 6
    launches = Launches(monkeypatch)
    got = replay(cuda_device, ref, ev, 7, launches)
    assert launches.count > 0
    assert_same_state(got, whole)


def test_entries_reject_an_empty_query_batch(cuda_device):
    """Why an empty range must launch nothing: the entries refuse nq < 1 (live buffers, so the size check is the one that speaks)."""
    from inclusivegan_amd import _abi, hip_ops
    dev = cuda_device
    q, c = torch.zeros(4, 5, device=dev), torch.zeros(6, 5, device=dev)
    qn, cn = torch.zeros(4, device=dev), torch.zeros(6, device=dev)
    rad = torch.zeros(6, 1, device=dev, dtype=torch.float64)
    member = torch.zeros(4, 1, device=dev, dtype=torch.int32)
    kth = hip_ops.knn_radius_state(4, 4, dev)
    d2, idx = hip_ops.nn1_state(4, dev)
    dots = torch.zeros(4, 6, device=dev)
    lib, P, S = _abi.get_plugin(), hip_ops._ptr, hip_ops._stream()
    for rc in (lib.igan_manifold_member_nn1_update(S, P(q), P(qn), P(c), P(cn), P(rad), P(member), P(d2), P(idx), P(dots), 0, 6, 5, 1, 0),
               lib.igan_manifold_member_update(S, P(q), P(qn), P(c), P(cn), P(rad), P(member), P(dots), 0, 6, 5, 1),
               lib.igan_knn_radius_update(S, P(q), P(qn), P(c), P(cn), P(kth), P(dots), 0, 6, 5, 4)):
        with pytest.raises(ValueError, match='sizes must be positive'):
            _abi.check(rc)


def test_one_process_evaluate_equals_the_two_call_form(cuda_device, big):
    """evaluate(return_realism, return_neighbors) takes membership and nearest neighbour from one product block; what it
    returns is what the pair of calls per batch gave before."""
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.metrics import precision_recall as PR
    ref, ev, whole = big
    dev = cuda_device
    rd, ed = torch.from_numpy(ref).to(dev), torch.from_numpy(ev).to(dev)
    m = PR.ManifoldEstimator(None, rd, ROW_BATCH, COL_BATCH, [K])
    got = m.evaluate(ed, return_realism=True, return_neighbors=True)

    rnorm = hip_ops.row_sqnorm_raw(rd)
    radii = torch.from_numpy(m.D).to(dev)
    member = torch.zeros((ed.shape[0], 1), device=dev, dtype=torch.int32)
    d2, idx = hip_ops.nn1_state(ed.shape[0], dev)
    for b1 in range(0, ed.shape[0], ROW_BATCH):
        rows = ed[b1:b1 + ROW_BATCH]
        norms = hip_ops.row_sqnorm_raw(rows)
        for b2 in range(0, rd.shape[0], COL_BATCH):
            hip_ops.manifold_member_update_raw(rows, norms, rd[b2:b2 + COL_BATCH], rnorm[b2:b2 + COL_BATCH], radii[b2:b2 + COL_BATCH], member[b1:b1 + ROW_BATCH])
            hip_ops.nn1_update_raw(rows, norms, rd[b2:b2 + COL_BATCH], rnorm[b2:b2 + COL_BATCH], d2[b1:b1 + ROW_BATCH], idx[b1:b1 + ROW_BATCH], b2)
    pred = member.cpu().numpy().astype(np.int32)
    nearest = idx.cpu().numpy().astype(np.int32)
    assert nearest.max() < ref.shape[0]
    with np.errstate(divide='ignore', invalid='ignore'):
        realism = (m.D[nearest, 0] / d2.cpu().numpy()).astype(np.float32)
    for name, a, b in zip(('predictions', 'realism', 'nearest'), got, (pred, realism, nearest)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    for name, a, b in zip(('predictions', 'realism', 'nearest'), got, (whole.precision, whole.realism_scores, whole.nearest_neighbors)):
        assert a.tobytes() == b.tobytes(), name
    # without the nearest neighbour the membership entry alone is called
    assert m.evaluate(ed).tobytes() == pred.tobytes()
