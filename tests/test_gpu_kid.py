"""GPU: the Kernel Inception Distance (metrics/kernel_inception_distance.py) against the brute force of tests/kid_oracle.py.

300 reals and 260 fakes at 48 features, 7 subsets of 100: the sums within the oracle's a-priori budget on the subsets that
kid_subsets returns, kid within the budget carried through the estimator; a subgroup of the reals by `real_rows` against the
physically sliced matrix, bit for bit; the ranks of a world replayed in one process and interleaved, as
test_gpu_density_coverage.py replays the row ranges; KID end to end on the HIP generator and through run_metrics."""
import functools
import os

import numpy as np
import pytest
import torch

import kid_oracle

pytestmark = pytest.mark.gpu

NUM_REAL, NUM_FAKE, F, S, CAP, SEED = 300, 260, 48, 7, 100, 3


def KIDM():
    from inclusivegan_amd.metrics import kernel_inception_distance
    return kernel_inception_distance


@functools.lru_cache(maxsize=None)
def recipe():
    """-> (reals, fakes, idx_fake, idx_real, oracle sums, bounds): non-negative features as a ReLU network gives them, the fakes
    a little off; shared, never written to."""
    rng = np.random.RandomState(21)
    real = np.maximum(rng.randn(NUM_REAL, F) + 0.5, 0).astype(np.float32)
    fake = np.maximum(rng.randn(NUM_FAKE, F) * 1.1 + 0.6, 0).astype(np.float32)
    idx_fake, idx_real, m = KIDM().kid_subsets(NUM_REAL, NUM_FAKE, S, CAP, SEED)
    assert m == CAP
    want, bound = kid_oracle.sums(fake, real, idx_fake, idx_real, 1.0 / F, 1.0)
    for a in (real, fake, idx_fake, idx_real, want, bound):
        a.setflags(write=False)
    return real, fake, idx_fake, idx_real, want, bound


def on_device(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


@functools.lru_cache(maxsize=None)
def whole():
    real, fake = recipe()[:2]
    dev = torch.device('cuda', 0)
    return KIDM().kid_from_features(on_device(real, dev), on_device(fake, dev), num_subsets=S, max_subset_size=CAP, seed=SEED)


def test_sums_and_kid_within_the_budget(cuda_device):
    real, fake, idx_fake, idx_real, want, bound = recipe()
    state = whole()
    assert state.m == CAP and state.sums.shape == (S, 3) and state.sums.dtype == np.float64 and state.per_subset.shape == (S,)
    err = np.abs(state.sums.astype(np.longdouble) - want.astype(np.longdouble)).astype(np.float64)
    assert np.all(err <= bound), (err / bound).max()
    want_kid, want_t = kid_oracle.kid_of_subsets(fake, real, idx_fake, idx_real)
    budget = kid_oracle.kid_bound(bound, CAP)
    print('kid %.9g oracle %.9g budget %.3g used %.3g' % (state.kid, want_kid, budget, abs(state.kid - want_kid) / budget))
    assert isinstance(state.kid, float) and abs(state.kid - want_kid) <= budget
    assert state.kid > 100 * budget                          # the two sets differ: the number is not its own error
    assert np.all(np.abs(state.per_subset - want_t) <= (bound[:, 0] + bound[:, 1]) / (CAP - 1) + 2 * bound[:, 2] / CAP)
    kid, per_subset = KIDM().kid_from_sums(state.sums, CAP)
    assert kid == state.kid and per_subset.tobytes() == state.per_subset.tobytes()
    # NumPy inputs: the same state
    host = KIDM().kid_from_features(np.array(real), np.array(fake), num_subsets=S, max_subset_size=CAP, seed=SEED)
    assert host.sums.tobytes() == state.sums.tobytes() and host.kid == state.kid
    with pytest.raises(ValueError):
        KIDM().kid_from_features(np.array(real), np.array(fake)[:, :40])
    with pytest.raises(ValueError):
        KIDM().kid_from_features(np.array(real), np.array(fake)[:1])


def test_identical_matrices_and_a_shifted_set(cuda_device):
    """The same matrix as reals and as fakes.  The unbiased estimator is NOT zero there, and is not meant to be: a subset pair
    drawn from one matrix shares rows, the cross sum counts k(x, x) of a shared row where the symmetric sums skip their diagonal,
    and two different draws differ by sampling noise (here kid = -0.036581 against a budget of 1.5e-11, and the extended-precision
    brute force gives the same -0.036581: "|kid| below the budget" cannot hold for a correct estimator).  What holds to the budget is the VALUE: kid equals the exact evaluation of
    the estimator on the same draws.  With the same rows at the same positions on both sides the value has a closed form --
    Kxx = Kyy = Kxy = K, t = 2 O / (m - 1) - 2 (O + D) / m with O the off-diagonal and D the diagonal sum of K -- and the kernel's
    sums give it within a small integer times the budget.  A fake set shifted by a constant gives kid > 0, far above the value
    for two samples of one law."""
    from inclusivegan_amd import hip_ops
    real = recipe()[0]
    rd = on_device(real, cuda_device)
    same = KIDM().kid_from_features(rd, rd, num_subsets=S, max_subset_size=CAP, seed=SEED)
    idx_a, idx_b, m = KIDM().kid_subsets(NUM_REAL, NUM_REAL, S, CAP, SEED)
    _, bound = kid_oracle.sums(real, real, idx_a, idx_b, 1.0 / F, 1.0)
    want = kid_oracle.kid_of_subsets(real, real, idx_a, idx_b)[0]
    budget = kid_oracle.kid_bound(bound, m)
    print('identical matrices: kid %.6g, exact %.6g, budget %.3g' % (same.kid, want, budget))
    assert abs(same.kid - want) <= budget
    # the same rows at the same positions
    sums = hip_ops.poly3_kernel_sums(rd, rd, idx_a, idx_a, 1.0 / F, 1.0).cpu().numpy()
    assert sums[:, 0].tobytes() == sums[:, 1].tobytes()
    off, bound = kid_oracle.sums(real, real, idx_a, idx_a, 1.0 / F, 1.0)
    diag, _ = kid_oracle.diagonal_sums(real, idx_a, 1.0 / F, 1.0)
    off, diag = off[:, 0].astype(np.longdouble), diag.astype(np.longdouble)
    closed = float(np.mean(2 * off / (m - 1) - 2 * (off + diag) / m) / m)
    kid = KIDM().kid_from_sums(sums, m)[0]
    assert closed < 0 and abs(kid - closed) <= 4 * kid_oracle.kid_bound(bound, m)
    # two samples of one law against a shifted one
    rng = np.random.RandomState(4)
    a = np.maximum(rng.randn(400, F) + 0.5, 0).astype(np.float32)
    b = np.maximum(rng.randn(400, F) + 0.5, 0).astype(np.float32)
    null = KIDM().kid_from_features(a, b, num_subsets=S, max_subset_size=CAP, seed=SEED)
    shifted = KIDM().kid_from_features(a, b + np.float32(0.25), num_subsets=S, max_subset_size=CAP, seed=SEED)
    print('kid of two samples of one law %.3g, of a shifted set %.3g' % (null.kid, shifted.kid))
    assert shifted.kid > 0 and shifted.kid > 10 * abs(null.kid)


def test_real_rows_equal_the_sliced_matrix(cuda_device):
    real, fake = recipe()[:2]
    rows = np.nonzero(np.random.RandomState(8).rand(NUM_REAL) < 0.3)[0]
    assert 60 < rows.size < 130
    rd, fd = on_device(real, cuda_device), on_device(fake, cuda_device)
    sub = KIDM().kid_from_features(rd, fd, num_subsets=S, max_subset_size=CAP, seed=SEED, real_rows=rows)
    cut = KIDM().kid_from_features(rd[torch.from_numpy(rows).to(cuda_device)], fd, num_subsets=S, max_subset_size=CAP, seed=SEED)
    assert sub.m == cut.m == rows.size
    assert sub.sums.tobytes() == cut.sums.tobytes() and sub.kid == cut.kid and sub.per_subset.tobytes() == cut.per_subset.tobytes()
    assert sub.sums.tobytes() != whole().sums.tobytes()
    for bad in (np.array([0, NUM_REAL]), np.array([-1, 3]), np.array([[0, 1]]), np.array([0.0, 1.0])):
        with pytest.raises(ValueError, match='real_rows'):
            KIDM().kid_from_features(rd, fd, num_subsets=S, max_subset_size=CAP, seed=SEED, real_rows=bad)
    with pytest.raises(ValueError, match='m - 1'):
        KIDM().kid_from_features(rd, fd, num_subsets=S, max_subset_size=CAP, seed=SEED, real_rows=rows[:1])


class Launches:
    """Counts the calls of hip_ops.poly3_kernel_sums."""

    def __init__(self, monkeypatch):
        from inclusivegan_amd import hip_ops
        self.count = 0
        orig = hip_ops.poly3_kernel_sums

        def counted(*args, **kwargs):
            self.count += 1
            return orig(*args, **kwargs)

        monkeypatch.setattr(hip_ops, 'poly3_kernel_sums', counted)


def replay(dev, world, launches):
    """The evaluation as the subsets of ranks 0 .. world - 1, each one launch (or none), put back in subset order."""
    kid = KIDM()
    real, fake, idx_fake, idx_real = recipe()[:4]
    rd, fd = on_device(real, dev), on_device(fake, dev)
    out = torch.full((S, 3), float('nan'), device=dev, dtype=torch.float64)
    seen = []
    for r in range(world):
        subsets = kid.rank_subsets(S, r, world)
        before = launches.count
        part = kid.kid_sums_rows(rd, fd, idx_fake, idx_real, subsets)
        assert launches.count == before + (1 if len(subsets) else 0)          # one launch per rank; none for a rank without subsets
        assert tuple(part.shape) == (len(subsets), 3) and part.dtype == torch.float64 and part.is_cuda
        for at, s in enumerate(subsets):
            out[int(s)] = part[at]
        seen += [int(s) for s in subsets]
    assert sorted(seen) == list(range(S))
    return out.cpu().numpy()


@pytest.mark.parametrize('world', [2, 3, 9])
def test_rank_replay_reassembles_the_one_process_sums(cuda_device, monkeypatch, world):
    state = whole()
    launches = Launches(monkeypatch)
    got = replay(cuda_device, world, launches)
    assert launches.count == min(world, S)
    assert got.tobytes() == state.sums.tobytes()
    assert KIDM().kid_from_sums(got, CAP)[0] == state.kid
    if world > S:
        assert [len(KIDM().rank_subsets(S, r, world)) for r in range(world)] == [1] * S + [0] * (world - S)


def _tiny_setup(tmp_path, dev, res=16):
    from inclusivegan_amd.dnnlib import tflib
    from inclusivegan_amd.training import misc, tfrecord
    kw = dict(num_channels=3, resolution=res, label_size=0, fmap_base=512, device=dev)
    G = tflib.Network('G', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', seed=41, **kw)
    D = tflib.Network('D', func_name='inclusivegan_amd.training.networks_stylegan2.D_stylegan2_feature', architecture='resnet', seed=42, **kw)
    pkl = str(tmp_path / 'network-snapshot-000001.pkl')
    misc.save_pkl((G, D, G.clone('Gs')), pkl)
    rng = np.random.RandomState(2)
    os.makedirs(str(tmp_path / 'data' / 'reals'))
    with tfrecord.TFRecordExporter(str(tmp_path / 'data' / 'reals'), 64, print_progress=False) as tfr:
        for _ in range(64):
            tfr.add_image(rng.randint(0, 256, size=(3, res, res)).astype(np.uint8))
    return pkl


def test_kid_reports_through_run_metrics(cuda_device, tmp_path, monkeypatch):
    """run_metrics with an injected feature network: metric-<name>.txt carries one value in %-10.6f (a tiny entry of the KID
    class; kid50k itself differs in its sizes alone)."""
    from inclusivegan_amd import run_metrics
    from inclusivegan_amd.dnnlib import EasyDict
    from inclusivegan_amd.metrics.metric_defaults import metric_defaults
    pkl = _tiny_setup(tmp_path, cuda_device)

    def feature_fn(images):
        return images.float().reshape(images.shape[0], 3, 4, 4, 4, 4).mean(dim=(3, 5)).reshape(images.shape[0], -1) / 64.0

    monkeypatch.setitem(metric_defaults, 'kid_tiny', EasyDict(dict(metric_defaults['kid50k'], name='kid_tiny', num_images=64, num_subsets=4,
                                                                   max_subset_size=40, minibatch_per_gpu=16)))
    run_dir = str(tmp_path / 'results' / '00000-run-metrics')
    group = run_metrics.run(pkl, ['kid_tiny'], dataset='reals', data_dir=str(tmp_path / 'data'), mirror_augment=False, run_dir=run_dir,
                            inject=dict(feature_fn=feature_fn, classify_fn=None))
    m = group.metrics[0]
    assert type(m) is KIDM().KID and (m.num_subsets, m.max_subset_size, m.seed) == (4, 40, 0)
    assert [(r.suffix, r.fmt) for r in m._results] == [('', '%-10.6f')]
    value = float(m._results[0].value)
    assert np.isfinite(value)
    assert m._real_features.shape == (64, 48) and m._real_features.is_cuda
    line = open(os.path.join(run_dir, 'metric-kid_tiny.txt')).read().splitlines()
    print(line)
    assert len(line) == 1 and line[0].endswith(('kid_tiny %-10.6f' % value).rstrip())
    with pytest.raises(RuntimeError, match='KID needs feature_fn'):
        run_metrics.run(pkl, ['kid_tiny'], dataset='reals', data_dir=str(tmp_path / 'data'), mirror_augment=False)


def test_kid_metric_on_the_hip_generator(cuda_device):
    """KID end to end: reals from the synthetic data set, fakes from Gs on the HIP path, injected feature network (a fixed random
    projection of the uint8 image); the reported number equals kid_from_features on the very same features."""
    from inclusivegan_amd.dnnlib import tflib
    kid = KIDM()
    dev = cuda_device
    Gs = tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', num_channels=3,
                       resolution=32, label_size=0, fmap_base=512, device=dev, seed=5)
    proj = torch.randn(3 * 32 * 32, 24, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) / 2000.0
    seen = dict(real=[], fake=[], real_done=False)

    def feature_fn(images):
        assert images.dtype == torch.uint8 and tuple(images.shape[1:]) == (3, 32, 32) and images.is_cuda
        f = images.float().reshape(images.shape[0], -1) @ proj
        seen['fake' if seen['real_done'] else 'real'].append(f.cpu().numpy())
        return f

    n = 200
    m = kid.KID(num_images=n, num_subsets=5, max_subset_size=64, minibatch_per_gpu=32, feature_fn=feature_fn, name='kid200')
    orig = m._generate
    m._generate = lambda *a, **k: (seen.__setitem__('real_done', True), orig(*a, **k))[1]
    m.run(Gs, dataset_args=dict(resolution=32, num_channels=3, label_size=0, data_size=256), mirror_augment=False, log_results=False)
    assert [(r.suffix, r.fmt) for r in m._results] == [('', '%-10.6f')]
    value = float(m._results[0].value)
    real, fake = np.concatenate(seen['real'])[:n], np.concatenate(seen['fake'])[:n]
    assert real.shape == (n, 24) and fake.shape == (n, 24)
    state = kid.kid_from_features(real, fake, num_subsets=5, max_subset_size=64, seed=0)
    assert state.m == 64 and value == state.kid
    idx_fake, idx_real, _ = kid.kid_subsets(n, n, 5, 64, 0)
    want, bound = kid_oracle.sums(fake, real, idx_fake, idx_real, 1.0 / 24, 1.0)
    err = np.abs(state.sums.astype(np.longdouble) - want.astype(np.longdouble)).astype(np.float64)
    assert np.all(err <= bound)
    assert abs(value - kid_oracle.kid_of_subsets(fake, real, idx_fake, idx_real)[0]) <= kid_oracle.kid_bound(bound, 64)
    assert ('kid200 %-10.6f' % value) in m.get_result_str()
    # real features are cached per object: a second run asks the feature network for fakes only
    calls = len(seen['real'])
    m._generate = orig
    seen['real_done'] = True
    m.run(Gs, dataset_args=dict(resolution=32, num_channels=3, label_size=0, data_size=256), mirror_augment=False, log_results=False)
    assert len(seen['real']) == calls and len(m._results) == 1 and np.isfinite(float(m._results[0].value))


def test_a_nan_feature_row_raises(cuda_device):
    real, fake = (np.array(a) for a in recipe()[:2])
    idx_fake = KIDM().kid_subsets(NUM_FAKE, NUM_FAKE, S, 20, SEED)[0]
    row = int(next(r for r in idx_fake[2] if r not in idx_fake[0] and r not in idx_fake[1]))     # subset 2 is the first to list it
    fake[row, 5] = np.nan
    for cap, first in ((NUM_FAKE, 0), (20, 2)):               # subsets of all 260 fakes; subsets of 20, of which 0 and 1 are clean
        m = KIDM().KID(num_images=NUM_FAKE, num_subsets=S, max_subset_size=cap, minibatch_per_gpu=32, seed=SEED, feature_fn=lambda images: images,
                       name='kidnan')
        m._feature_matrix = lambda Gs, Gs_kwargs, which, num_gpus: on_device(real[:NUM_FAKE] if which == 'real' else fake, cuda_device)
        with pytest.raises(FloatingPointError, match='subset %d ' % first):
            m._evaluate(None, {}, 1)
