"""GPU: density and coverage (metrics/density_coverage.py) against the fp64 brute force of tests/dc_oracle.py.

The recipe is that of tests/test_gpu_pr_shards.py -- 203 reals and 190 fakes at 24 features with duplicates inside the reals,
across the sets and inside the fakes -- plus one planted row: fake 7 is a bit copy of the k-th neighbour of real 30, so it lies
exactly ON real 30's sphere (outside by the strict comparison).  Radii are compared by tobytes() with ManifoldEstimator's,
counts as integers, density and coverage with ==.  The row-range form of the count pass is replayed for every rank of a world in
one process and concatenated, as test_gpu_pr_shards.py does for the four passes of pr50k3."""
import functools

import numpy as np
import pytest
import torch

import dc_oracle
import test_gpu_pr_shards
from test_gpu_pr_shards import make_features

pytestmark = pytest.mark.gpu

ROW_BATCH, COL_BATCH = 64, 50

# (density, coverage, inclusive density) of the recipe, computed once from the oracle on the host: a cross-check of the recipe,
# the tests recompute them
LITERALS = {5: (0.66, 0.9211822660098522, 0.6621052631578948),
            3: (0.631578947368421, 0.729064039408867, 0.6350877192982456),
            1: (0.5842105263157895, 0.35467980295566504, 0.6263157894736842)}


def DCM():
    from inclusivegan_amd.metrics import density_coverage
    return density_coverage


@functools.lru_cache(maxsize=None)
def recipe(k):
    """-> (reals, fakes, oracle strict, oracle inclusive) for neighbourhood k; decided (dc_oracle.assert_decided); shared, never written to."""
    real, fake = make_features(203, 190, 24, 11)
    d30 = dc_oracle.exact_sqdist(real[30:31], real)[0]
    fake[7] = real[int(np.argsort(d30, kind='stable')[k])]
    strict = dc_oracle.density_coverage(real, fake, [k])
    inclusive = dc_oracle.density_coverage(real, fake, [k], inclusive=True)
    assert strict['d2'][30, 7] == strict['radii'][30, 0] and dc_oracle.exact_ties(strict['d2'], strict['radii']) >= 2
    for a in (real, fake, strict['radii'], strict['d2'], strict['counts'], inclusive['counts']):
        a.setflags(write=False)
    return real, fake, strict, inclusive


def on_device(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


@functools.lru_cache(maxsize=None)
def whole(k):
    """density_coverage_features of the recipe at neighbourhood k, computed once."""
    real, fake, _, _ = recipe(k)
    dev = torch.device('cuda', 0)
    return DCM().density_coverage_features(on_device(real, dev), on_device(fake, dev), nhood_sizes=[k], row_batch_size=ROW_BATCH, col_batch_size=COL_BATCH)


@pytest.mark.parametrize('k', [1, 3, 5])
def test_density_and_coverage_equal_the_oracle(cuda_device, k):
    from inclusivegan_amd.metrics import precision_recall
    dc = DCM()
    real, fake, strict, inclusive = recipe(k)
    assert (strict['density'][0], strict['coverage'][0], inclusive['density'][0]) == LITERALS[k]
    state = whole(k)
    m = precision_recall.ManifoldEstimator(None, on_device(real, cuda_device), ROW_BATCH, COL_BATCH, [k])
    assert state.radii.dtype == np.float64 and state.radii.shape == (203, 1) and state.radii.tobytes() == m.D.tobytes()
    assert np.all(np.abs(state.radii - strict['radii']) <= 1e-11 * strict['radii'])
    assert state.counts.dtype == np.int64 and state.counts.shape == (203, 1) and np.array_equal(state.counts, strict['counts'])
    print('k %d density %r coverage %r' % (k, float(state.density[0]), float(state.coverage[0])))
    assert state.density.shape == (1,) and state.coverage.shape == (1,)
    assert float(state.density[0]) == strict['density'][0] and float(state.coverage[0]) == strict['coverage'][0]
    # the fake ON real 30's sphere is outside strictly and inside inclusively
    got_inclusive = dc.ball_counts_rows(on_device(real, cuda_device), state.radii, on_device(fake, cuda_device), 0, 203, ROW_BATCH, COL_BATCH,
                                        inclusive=True).cpu().numpy()
    assert np.array_equal(got_inclusive, inclusive['counts'])
    assert got_inclusive[30, 0] > state.counts[30, 0]
    assert int(got_inclusive.sum()) / (k * 190) == inclusive['density'][0]
    if k == 1:      # the duplicated reals 17 and 101 have radius 0: nothing is strictly inside, not even fake 5, their copy
        assert state.radii[17, 0] == 0 and state.radii[101, 0] == 0 and np.array_equal(fake[5], real[17])
        assert state.counts[17, 0] == 0 and state.counts[101, 0] == 0 and got_inclusive[17, 0] == 1 and got_inclusive[101, 0] == 1


def test_several_neighbourhood_sizes_inputs_and_batch_sizes(cuda_device):
    dc = DCM()
    real, fake, strict, _ = recipe(3)                 # the sphere of real 30 at k = 3 carries the planted fake
    ks = [1, 3, 5]
    both = dc.density_coverage_features(on_device(real, cuda_device), on_device(fake, cuda_device), nhood_sizes=ks, row_batch_size=ROW_BATCH,
                                        col_batch_size=COL_BATCH)
    want = dc_oracle.density_coverage(real, fake, ks)
    assert both.radii.shape == (203, 3) and np.array_equal(both.counts, want['counts'])
    assert both.density.tolist() == want['density'] and both.coverage.tolist() == want['coverage']
    one = whole(3)
    assert both.radii[:, 1].tobytes() == one.radii[:, 0].tobytes() and np.array_equal(both.counts[:, 1], one.counts[:, 0])
    assert both.density[1] == one.density[0] and both.coverage[1] == one.coverage[0]
    # NumPy inputs, and other batch sizes: the same state
    for args in (dict(row_batch_size=ROW_BATCH, col_batch_size=COL_BATCH), dict(row_batch_size=1000, col_batch_size=1000)):
        other = dc.density_coverage_features(np.array(real), np.array(fake), nhood_sizes=ks, **args)
        assert other.radii.tobytes() == both.radii.tobytes() and other.counts.tobytes() == both.counts.tobytes()
        assert other.density.tobytes() == both.density.tobytes() and other.coverage.tobytes() == both.coverage.tobytes()
    with pytest.raises(ValueError):
        dc.density_coverage_features(np.array(real), np.array(fake), nhood_sizes=[0])
    with pytest.raises(ValueError):
        dc.density_coverage_features(np.array(real), np.array(fake)[:, :20])


class Launches(test_gpu_pr_shards.Launches):
    """Counts the calls of the search wrappers that the count pass makes."""
    NAMES = ('row_sqnorm_raw', 'knn_radius_update_raw', 'ball_count_update_raw')


def replay(dev, real, fake, radii, world, launches=None):
    """The count pass as the row ranges of ranks 0 .. world - 1, concatenated in rank order."""
    from inclusivegan_amd.metrics import precision_recall
    dc = DCM()
    rd, fd = on_device(real, dev), on_device(fake, dev)
    parts = []
    for r in range(world):
        b, e = precision_recall.search_rows(real.shape[0], r, world)
        before = launches.count if launches else 0
        part = dc.ball_counts_rows(rd, radii, fd, b, e, ROW_BATCH, COL_BATCH)
        if launches and e == b:
            assert launches.count == before                  # an empty range launches nothing
        assert part.shape == (e - b, radii.shape[1]) and part.dtype == torch.int64 and part.is_cuda
        parts.append(part)
    return torch.cat(parts).cpu().numpy()


@pytest.mark.parametrize('world', [1, 2, 3, 7])
def test_row_shards_concatenate_to_the_whole_pass(cuda_device, world):
    real, fake, _, _ = recipe(5)
    state = whole(5)
    got = replay(cuda_device, real, fake, state.radii, world)
    assert got.dtype == state.counts.dtype and got.tobytes() == state.counts.tobytes()
    assert 0 < state.coverage[0] < 1 and 0 < state.density[0]


def test_ranks_without_rows_launch_nothing(cuda_device, monkeypatch):
    from inclusivegan_amd.metrics import precision_recall
    dc = DCM()
    real, fake = make_features(6, 6, 24, 12)
    state = dc.density_coverage_features(on_device(real, cuda_device), on_device(fake, cuda_device), nhood_sizes=[3], row_batch_size=ROW_BATCH,
                                         col_batch_size=COL_BATCH)
    assert np.array_equal(state.counts, dc_oracle.density_coverage(real, fake, [3])['counts'])
    assert [precision_recall.search_rows(6, r, 7) for r in range(7)].count((0, 0)) == 1     # rank 0 of 7 owns no row of 6
    launches = Launches(monkeypatch)
    got = replay(cuda_device, real, fake, state.radii, 7, launches)
    assert launches.count > 0
    assert got.tobytes() == state.counts.tobytes()


def test_dc_reports_through_run_metrics(cuda_device, tmp_path, monkeypatch):
    """run_metrics with an injected feature network: metric-<name>.txt carries both numbers (a tiny entry of the DC class; dc50k5
    itself differs in its sizes alone)."""
    import os
    from inclusivegan_amd import run_metrics
    from inclusivegan_amd.dnnlib import EasyDict, tflib
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    from inclusivegan_amd.training import misc, tfrecord
    res = 16
    kw = dict(num_channels=3, resolution=res, label_size=0, fmap_base=512, device=cuda_device)
    G = tflib.Network('G', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', seed=41, **kw)
    D = tflib.Network('D', func_name='inclusivegan_amd.training.networks_stylegan2.D_stylegan2_feature', architecture='resnet', seed=42, **kw)
    pkl = str(tmp_path / 'network-snapshot-000001.pkl')
    misc.save_pkl((G, D, G.clone('Gs')), pkl)
    rng = np.random.RandomState(2)
    os.makedirs(str(tmp_path / 'data' / 'reals'))
    with tfrecord.TFRecordExporter(str(tmp_path / 'data' / 'reals'), 64, print_progress=False) as tfr:
        for _ in range(64):
            tfr.add_image(rng.randint(0, 256, size=(3, res, res)).astype(np.uint8))

    def feature_fn(images):
        return images.float().reshape(images.shape[0], 3, 4, 4, 4, 4).mean(dim=(3, 5)).reshape(images.shape[0], -1)

    monkeypatch.setitem(metric_defaults, 'dc_tiny', EasyDict(dict(metric_defaults['dc50k5'], name='dc_tiny', num_images=64, minibatch_per_gpu=16,
                                                                  row_batch_size=40, col_batch_size=24)))
    run_dir = str(tmp_path / 'results' / '00000-run-metrics')
    group = run_metrics.run(pkl, ['dc_tiny'], dataset='reals', data_dir=str(tmp_path / 'data'), mirror_augment=False, run_dir=run_dir,
                            inject=dict(feature_fn=feature_fn, classify_fn=None))
    m = group.metrics[0]
    assert type(m) is DCM().DC and m.nhood_size == 5 and [r.suffix for r in m._results] == ['_density', '_coverage']
    density, coverage = (float(r.value) for r in m._results)
    assert density >= 0.0 and 0.0 <= coverage <= 1.0
    assert m._real_features.shape == (64, 48) and m._real_features.is_cuda
    line = open(os.path.join(run_dir, 'metric-dc_tiny.txt')).read().splitlines()
    assert len(line) == 1 and line[0].endswith(('dc_tiny_density %-10.4f dc_tiny_coverage %-10.4f' % (density, coverage)).rstrip())
    with pytest.raises(RuntimeError, match='DC needs feature_fn'):
        run_metrics.run(pkl, ['dc_tiny'], dataset='reals', data_dir=str(tmp_path / 'data'), mirror_augment=False)


def test_dc_metric_on_the_hip_generator(cuda_device):
    """DC end to end: reals from the synthetic data set, fakes from Gs on the HIP path, injected feature network (a fixed random
    projection of the uint8 image); the two reported numbers equal density_coverage_features on the very same features."""
    from inclusivegan_amd.dnnlib import tflib
    dc = DCM()
    dev = cuda_device
    Gs = tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', num_channels=3,
                       resolution=32, label_size=0, fmap_base=512, device=dev, seed=5)
    proj = torch.randn(3 * 32 * 32, 24, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) / 55.0
    seen = dict(real=[], fake=[], real_done=False)

    def feature_fn(images):
        assert images.dtype == torch.uint8 and tuple(images.shape[1:]) == (3, 32, 32) and images.is_cuda
        f = images.float().reshape(images.shape[0], -1) @ proj
        seen['fake' if seen['real_done'] else 'real'].append(f.cpu().numpy())
        return f

    n = 200
    m = dc.DC(num_images=n, nhood_size=5, minibatch_per_gpu=32, row_batch_size=64, col_batch_size=64, feature_fn=feature_fn, name='dc200')
    orig = m._generate
    m._generate = lambda *a, **k: (seen.__setitem__('real_done', True), orig(*a, **k))[1]
    m.run(Gs, dataset_args=dict(resolution=32, num_channels=3, label_size=0, data_size=256), mirror_augment=False, log_results=False)
    assert [r.suffix for r in m._results] == ['_density', '_coverage']
    values = [float(r.value) for r in m._results]
    assert values[0] >= 0.0 and 0.0 <= values[1] <= 1.0
    real, fake = np.concatenate(seen['real'])[:n], np.concatenate(seen['fake'])[:n]
    assert real.shape == (n, 24) and fake.shape == (n, 24)
    state = dc.density_coverage_features(real, fake, nhood_sizes=[5], row_batch_size=64, col_batch_size=64)
    assert values == [float(state.density[0]), float(state.coverage[0])]
    want = dc_oracle.density_coverage(real, fake, [5])
    assert np.array_equal(state.counts, want['counts'])
    assert 'dc200_density' in m.get_result_str() and 'dc200_coverage' in m.get_result_str()
    # real features are cached per object: a second run asks the feature network for fakes only
    calls = len(seen['real'])
    m._generate = orig
    seen['real_done'] = True
    m.run(Gs, dataset_args=dict(resolution=32, num_channels=3, label_size=0, data_size=256), mirror_augment=False, log_results=False)
    assert len(seen['real']) == calls and len(m._results) == 2
