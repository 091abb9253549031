"""CPU: pr50k3, prd30k and the path lengths on every rank -- the parts that need no device.  Which metrics spread, the new
entry igan_manifold_member_nn1_update in the header, the binding and its argument checks, the row ranges of the sharded
search, the dealing of PPL's minibatches, and the refusal of host features under a process group."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_which_metrics_spread_over_the_ranks():
    from inclusivegan_amd.metrics import linear_separability, metric_base, perceptual_path_length, prd_score, precision_recall
    assert precision_recall.PR.multi_rank is True
    assert prd_score.PRD.multi_rank is True
    assert perceptual_path_length.PPL.multi_rank is True
    assert linear_separability.LS.multi_rank is False
    assert metric_base.MetricBase.multi_rank is False


def test_header_and_binding_of_the_new_entry():
    from inclusivegan_amd import _abi
    header = open(os.path.join(ROOT, 'include', 'igan_hip.h')).read()
    m = re.search(r'\bint\s+igan_manifold_member_nn1_update\s*\(([^;]*)\)\s*;', header)
    assert m is not None
    params = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')
    assert len(params) == 15
    assert params[-1].split()[-1] == 'idx_base' and params[-2].split()[-1] == 'nk'
    lib = _abi.get_plugin()
    fn = lib.igan_manifold_member_nn1_update
    assert len(fn.argtypes) == 15
    assert list(fn.argtypes[-5:]) == [ctypes.c_int] * 5 and fn.restype is ctypes.c_int
    assert _abi.ABI_VERSION == 10 and lib.igan_abi_version() == 10
    assert re.search(r'#define\s+IGAN_ABI_VERSION\s+10\b', header)


def test_new_entry_validates_without_a_device():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    P = 1 << 20           # never dereferenced: validation fails first
    bad = _abi.IGAN_ERR_INVALID_ARGUMENT
    INT32_MAX = 2 ** 31 - 1

    def both(query=P, qnorm=P, cand=P, cnorm=P, radii=P, flags=P, best_d2=P, best_idx=P, dots=P, nq=4, nc=64, dim=16, nk=1, idx_base=0):
        return lib.igan_manifold_member_nn1_update(None, query, qnorm, cand, cnorm, radii, flags, best_d2, best_idx, dots, nq, nc, dim, nk, idx_base)

    for b in ('query', 'qnorm', 'cand', 'cnorm', 'radii', 'flags', 'best_d2', 'best_idx', 'dots'):
        assert both(**{b: None}) == bad, b
        assert b'null buffer' in lib.igan_last_error()
    for size in ('nq', 'nc', 'dim'):
        for v in (0, -3):
            assert both(**{size: v}) == bad, size
            assert b'sizes must be positive' in lib.igan_last_error()
    assert both(nq=1 << 20, dim=1 << 10) == bad and b'2 GiB' in lib.igan_last_error()
    assert both(nc=1 << 20, dim=1 << 10) == bad and b'2 GiB' in lib.igan_last_error()
    assert both(nq=1 << 16, nc=1 << 16, dim=4) == bad and b'too large' in lib.igan_last_error()
    for nk in (0, 9, -1):
        assert both(nk=nk) == bad and b'nk' in lib.igan_last_error()
    for base in (-1, INT32_MAX - 63, INT32_MAX):
        assert both(idx_base=base) == bad and b'overflows int32' in lib.igan_last_error()
    # the same words, the same codes as the two entries it stands for
    assert lib.igan_nn1_update(None, P, P, P, P, P, P, P, 4, 64, 16, INT32_MAX - 63) == bad and b'overflows int32' in lib.igan_last_error()
    assert lib.igan_manifold_member_update(None, P, P, P, P, P, P, P, 4, 64, 16, 9) == bad and b'nk' in lib.igan_last_error()


def test_wrapper_has_no_cpu_path():
    import torch
    from inclusivegan_amd import hip_ops
    q = torch.zeros(4, 8)
    d2, idx = hip_ops.nn1_state(4, 'cpu')
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.manifold_member_nn1_update_raw(q, torch.zeros(4), q, torch.zeros(4), torch.zeros(4, 1, dtype=torch.float64),
                                               torch.zeros(4, 1, dtype=torch.int32), d2, idx, 0)


@pytest.mark.parametrize('n', [0, 1, 5, 203])
@pytest.mark.parametrize('world', [1, 2, 3, 7])
def test_search_rows_partition(n, world):
    from inclusivegan_amd.metrics.precision_recall import search_rows
    ranges = [search_rows(n, r, world) for r in range(world)]
    assert ranges[0][0] == 0 and ranges[-1][1] == n
    for (b, e), (b2, _) in zip(ranges, ranges[1:] + [(n, n)]):
        assert 0 <= b <= e <= n and e == b2          # ordered, disjoint, no gap
    lengths = [e - b for b, e in ranges]
    assert sum(lengths) == n and max(lengths) - min(lengths) <= 1
    with pytest.raises(ValueError):
        search_rows(n, world, world)


@pytest.mark.parametrize('T', [1, 5, 10])
@pytest.mark.parametrize('world', [1, 2, 3])
def test_ppl_minibatches_have_one_owner(T, world):
    from inclusivegan_amd.metrics.perceptual_path_length import minibatches_of_rank, num_minibatches
    mine = [minibatches_of_rank(T, r, world) for r in range(world)]
    owners = {}
    for r, gs in enumerate(mine):
        for i, g in enumerate(gs):
            assert g not in owners and g % world == r and g // world == i
            owners[g] = r
    assert sorted(owners) == list(range(T))
    # re-interleaving the per-rank lists, round by round, gives 0 .. T - 1
    back = [mine[g % world][g // world] for g in range(T)]
    assert back == list(range(T))
    assert num_minibatches(10, 2) == 5 and num_minibatches(9, 2) == 5 and num_minibatches(1, 8) == 1


def test_ppl_distances_takes_a_process_group():
    import inspect
    from inclusivegan_amd.metrics import perceptual_path_length, precision_recall
    assert inspect.signature(perceptual_path_length.PPL.distances).parameters['process_group'].default is None
    assert inspect.signature(precision_recall.knn_precision_recall_features).parameters['process_group'].default is None
    assert inspect.signature(precision_recall.ManifoldEstimator.__init__).parameters['process_group'].default is None


SYNTHETIC = dict(resolution=32, num_channels=3, label_size=0, data_size=32)


@pytest.mark.parametrize('which', ['PR', 'PRD'])
@pytest.mark.parametrize('returns', ['numpy', 'cpu_tensor'])
def test_host_features_are_refused_under_a_group(which, returns):
    """As FID refuses them: a rank's rows must stay on the device to be gathered.  The rows of a rank are a function of
    (rank, world), so the refusal shows without a process group's collectives."""
    import torch
    from inclusivegan_amd.metrics import prd_score, precision_recall

    def feature_fn(images):
        f = np.zeros((images.shape[0], 6), np.float32)
        return f if returns == 'numpy' else torch.from_numpy(f)

    if which == 'PR':
        m = precision_recall.PR(num_images=12, nhood_size=3, minibatch_per_gpu=4, row_batch_size=8, col_batch_size=8, feature_fn=feature_fn, name='pr_t')
    else:
        m = prd_score.PRD(num_images=12, num_clusters=2, num_angles=11, num_runs=1, minibatch_per_gpu=4, feature_fn=feature_fn, name='prd_t')
    m._configure('live-network', None, dict(SYNTHETIC), False)
    Gs = types.SimpleNamespace(device=torch.device('cpu'))
    try:
        with pytest.raises(RuntimeError, match='must return device tensors'):
            m._shard_feature_rows(Gs, {}, 'real', 1, 2)
    finally:
        m.close()
