"""GPU: FID statistics on the device (csrc/moments.hip).  igan_moments_update against fp64 / extended-precision NumPy on the
same fp32 rows -- EQUAL on integer data (every partial sum is exact, so a wrong fragment map, a transposed or permuted store
or a lost row cannot pass), within the worst-case bound of an n-term fp64 sum on float data, bit-identical when repeated,
isolated propagation of one non-finite element; igan_moments_finalize and FeatureMoments against a two-pass extended-precision
covariance; the FID class on the device path against the host formula on the very same features, the unchanged host path, the
non-finite error and the reference's on-disk cache of real statistics."""
import os

import numpy as np
import pytest
import torch

import fid_oracle as O

pytestmark = pytest.mark.gpu

INT_SHAPES = [(1, 1), (3, 17), (5, 16), (64, 65), (257, 50), (1000, 130)]


def hip_moments(X, shift, dev, chunk=None, state=None):
    """-> (sum [F], gram [F, F]) as NumPy arrays after folding X (NumPy fp32 or a device tensor) in chunks of `chunk` rows."""
    from inclusivegan_amd import hip_ops
    Xd = torch.from_numpy(X).to(dev) if isinstance(X, np.ndarray) else X
    n, F = Xd.shape
    sh = None if shift is None else torch.from_numpy(np.asarray(shift, dtype=np.float64)).to(dev)
    s, g = state if state is not None else (torch.zeros(F, device=dev, dtype=torch.float64), torch.zeros((F, F), device=dev, dtype=torch.float64))
    step = n if chunk is None else chunk
    for r0 in range(0, n, step):
        hip_ops.moments_update_raw(Xd[r0:r0 + step], sh, s, g)
    return s.cpu().numpy(), g.cpu().numpy()


def upper(F):
    return np.triu(np.ones((F, F), dtype=bool))


@pytest.mark.parametrize('shift_value', [None, 3.0])
@pytest.mark.parametrize('n,F', INT_SHAPES)
def test_update_is_exact_on_integer_rows(cuda_device, n, F, shift_value):
    X = O.integer_rows(n, F)
    shift = None if shift_value is None else np.full(F, shift_value)
    want_sum, want_gram = O.moments_fp64(X, shift)                       # integers below 2^53: exact in any order
    up = upper(F)
    got_sum, got_gram = hip_moments(X, shift, cuda_device)
    assert np.array_equal(got_sum, want_sum)
    assert np.array_equal(got_gram[up], want_gram[up])
    chunked_sum, chunked_gram = hip_moments(X, shift, cuda_device, chunk=100)
    assert np.array_equal(chunked_sum, want_sum) and np.array_equal(chunked_gram[up], want_gram[up])
    again_sum, again_gram = hip_moments(X, shift, cuda_device, chunk=100)
    assert again_sum.tobytes() == chunked_sum.tobytes() and again_gram.tobytes() == chunked_gram.tobytes()


def test_update_accumulates_into_running_statistics(cuda_device):
    """Two different batches into one state: the second call adds to what the first left (sum and every upper-triangle tile)."""
    A, B = O.integer_rows(70, 130), O.integer_rows(33, 130)[:, ::-1].copy()
    dev = cuda_device
    state = (torch.zeros(130, device=dev, dtype=torch.float64), torch.zeros((130, 130), device=dev, dtype=torch.float64))
    hip_moments(A, None, dev, state=state)
    got_sum, got_gram = hip_moments(B, None, dev, state=state)
    want_sum, want_gram = O.moments_fp64(np.concatenate([A, B]), None)
    assert np.array_equal(got_sum, want_sum) and np.array_equal(got_gram[upper(130)], want_gram[upper(130)])


@pytest.mark.parametrize('n,F', [(5000, 64), (333, 50), (1000, 2048), (64, 4096)])
def test_update_meets_the_fp64_sum_bound_on_float_rows(cuda_device, n, F):
    """|gram - oracle| <= n 2^-50 sqrt(M_jj M_kk) and |sum - oracle| <= n 2^-50 sqrt(n M_jj).  The oracle is np.longdouble: the whole
    upper triangle at the small widths, the tile-edge rows and a seeded sample of rows at 2048 / 4096 (an extended-precision
    product is not a BLAS call), where every entry is checked against the fp64 BLAS product under the same bound as well --
    that is what its factor 4 is for."""
    X = O.float_rows(n, F, seed=n + F)
    shift = O.first_rows_shift(X)
    got_sum, got_gram = hip_moments(X, shift, cuda_device)
    rows = None if F <= 64 else O.edge_rows(F)
    want_sum, want_rows = O.moments_longdouble(X, shift, rows)
    rows = np.arange(F) if rows is None else rows
    blas_sum, blas_gram = O.moments_fp64(X, shift)
    diag = np.diagonal(blas_gram)
    bound = O.gram_bound(n, diag)
    keep = rows[:, None] <= np.arange(F)[None, :]                        # the upper-triangle part of the checked rows
    err = np.abs((got_gram[rows].astype(np.longdouble) - want_rows).astype(np.float64))
    err_blas = np.abs(got_gram - blas_gram)
    err_sum = np.abs((got_sum.astype(np.longdouble) - want_sum).astype(np.float64))
    print('(%d, %d): gram err / bound max %.3e (longdouble rows) %.3e (fp64 BLAS, all); sum err / bound max %.3e'
          % (n, F, float(np.max((err / bound[rows])[keep])), float(np.max((err_blas / bound)[upper(F)])), float(np.max(err_sum / O.sum_bound(n, diag)))))
    assert np.all(diag > 0)
    assert np.all(err[keep] <= bound[rows][keep])
    assert np.all(err_blas[upper(F)] <= bound[upper(F)])
    assert np.all(err_sum <= O.sum_bound(n, diag))


def test_update_reads_a_view_that_starts_at_an_odd_row(cuda_device):
    """X needs 4-byte alignment only: rows 1 .. of an F = 50 allocation start 200 bytes in."""
    X = O.float_rows(258, 50, seed=5)
    shift = O.first_rows_shift(X[1:])
    whole = torch.from_numpy(X).to(cuda_device)
    view = whole[1:]
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    got = hip_moments(view, shift, cuda_device)
    want = hip_moments(view.clone(), shift, cuda_device)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize('poison', [float('nan'), float('inf')])
def test_one_non_finite_element_reaches_its_row_and_column_only(cuda_device, poison):
    n, F, i, j = 300, 130, 77, 70
    X = O.float_rows(n, F, seed=9)
    shift = O.first_rows_shift(X)
    clean_sum, clean_gram = hip_moments(X, shift, cuda_device)
    X[i, j] = poison
    got_sum, got_gram = hip_moments(X, shift, cuda_device)
    up = upper(F)
    touched = np.zeros((F, F), dtype=bool)
    touched[j, :] = touched[:, j] = True
    assert not np.isfinite(got_sum[j]) and not np.any(np.isfinite(got_gram[touched & up]))
    others = np.arange(F) != j
    assert got_sum[others].tobytes() == clean_sum[others].tobytes()
    assert got_gram[up & ~touched].tobytes() == clean_gram[up & ~touched].tobytes()
    assert np.all(np.isfinite(clean_gram[up])) and np.all(np.isfinite(clean_sum))


@pytest.mark.parametrize('n,F', [(5000, 64), (333, 50)])
def test_finalize_meets_the_bound_and_is_symmetric(cuda_device, n, F):
    from inclusivegan_amd import hip_ops
    X = O.float_rows(n, F, seed=2 * n + F)
    shift = O.first_rows_shift(X)
    dev = cuda_device
    shd = torch.from_numpy(shift).to(dev)
    s, g = torch.zeros(F, device=dev, dtype=torch.float64), torch.zeros((F, F), device=dev, dtype=torch.float64)
    hip_ops.moments_update_raw(torch.from_numpy(X).to(dev), shd, s, g)
    mean, cov = (t.cpu().numpy() for t in hip_ops.moments_finalize_raw(s, g, shd, n))
    assert cov.tobytes() == cov.T.copy().tobytes()
    want_mean, want_cov = O.mean_cov_longdouble(X)
    diag = np.diagonal(O.moments_fp64(X, shift)[1])
    cov_bound = O.gram_bound(n, diag) / (n - 1)
    mean_bound = O.EPS50 * np.sqrt(n * diag)
    err_cov = np.abs((cov.astype(np.longdouble) - want_cov).astype(np.float64))
    err_mean = np.abs((mean.astype(np.longdouble) - want_mean).astype(np.float64))
    np_cov = np.abs((np.cov(X, rowvar=False).astype(np.longdouble) - want_cov).astype(np.float64))
    print('(%d, %d): cov err / bound max %.3e, np.cov %.3e; mean err / bound max %.3e'
          % (n, F, float(np.max(err_cov / cov_bound)), float(np.max(np_cov / cov_bound)), float(np.max(err_mean / mean_bound))))
    assert np.all(err_cov <= cov_bound) and np.all(err_mean <= mean_bound)
    assert np.all(np_cov <= cov_bound)                                   # the bound is one np.cov itself meets
    # finalize writes: a second call into poisoned outputs gives the same bits, and a NULL shift means 0
    mean2, cov2 = (t.cpu().numpy() for t in hip_ops.moments_finalize_raw(s, g, shd, n))
    assert mean2.tobytes() == mean.tobytes() and cov2.tobytes() == cov.tobytes()
    Xi = O.integer_rows(37, F)
    si, gi = torch.zeros(F, device=dev, dtype=torch.float64), torch.zeros((F, F), device=dev, dtype=torch.float64)
    hip_ops.moments_update_raw(torch.from_numpy(Xi).to(dev), None, si, gi)
    mean_i, cov_i = (t.cpu().numpy() for t in hip_ops.moments_finalize_raw(si, gi, None, 37))
    D = Xi.astype(np.float64)
    S, G = D.sum(axis=0), D.T @ D
    assert np.array_equal(mean_i, S / 37.0) and np.array_equal(cov_i, (G - S[:, None] * S[None, :] / 37.0) / 36.0)


def test_feature_moments_constant_columns_and_count(cuda_device):
    from inclusivegan_amd import hip_ops
    n, F = 250, 70
    X = O.float_rows(n, F, seed=4)
    consts = {0: 0.0, 5: 1.5, 63: np.float32(0.1), 64: -7.25, 69: np.float32(1e-3)}
    for c, v in consts.items():
        X[:, c] = v
    fm = hip_ops.FeatureMoments(F, cuda_device, chunk_rows=64)
    for r0 in range(0, n, 24):                                           # 24-row batches against 64-row chunks: every split position
        fm.update(torch.from_numpy(X[r0:r0 + 24]).to(cuda_device))
    assert fm.count == n
    mu, sigma = fm.finalize()
    assert mu.dtype == np.float64 and sigma.dtype == np.float64 and mu.shape == (F,) and sigma.shape == (F, F)
    for c, v in consts.items():
        assert mu[c] == float(v), c
        assert not np.any(sigma[c, :]) and not np.any(sigma[:, c]), c
    shift = fm.shift.cpu().numpy()
    first = X[:24].astype(np.float64)                                    # the first batch's fp64 column mean, in whatever order it was added
    assert np.all(np.abs(shift - first.mean(axis=0)) <= 24 * 2.0 ** -52 * np.abs(first).mean(axis=0))
    want_mean, want_cov = O.mean_cov_longdouble(X)
    bound = O.gram_bound(n, np.diagonal(O.moments_fp64(X, shift)[1])) / (n - 1)          # the finalize bound; 0 in the constant columns
    assert np.all(np.abs((sigma.astype(np.longdouble) - want_cov).astype(np.float64)) <= bound)
    # double features are staged as fp32: the same rows in one 250-row batch give the chunked result of that batch order
    fh = hip_ops.FeatureMoments(F, cuda_device, chunk_rows=64)
    for r0 in range(0, n, 24):
        fh.update(torch.from_numpy(X[r0:r0 + 24]).to(cuda_device).double())
    mu_d, sigma_d = fh.finalize()
    assert mu_d.tobytes() == mu.tobytes() and sigma_d.tobytes() == sigma.tobytes()
    with pytest.raises(ValueError):
        fh.update(torch.zeros(4, F + 1, device=cuda_device))
    with pytest.raises(RuntimeError, match='no CPU path'):
        fh.update(torch.zeros(4, F))


def test_feature_moments_on_offset_data(cuda_device):
    """100 + 0.01 N(0, 1): a zero shift loses 3.6e-7 of sqrt(cov_jj cov_kk) to cancellation; the first-batch shift must not."""
    from inclusivegan_amd import hip_ops
    n, F = 5000, 64
    X = (100.0 + 0.01 * np.random.RandomState(11).randn(n, F)).astype(np.float32)
    fm = hip_ops.FeatureMoments(F, cuda_device, chunk_rows=1024)
    for r0 in range(0, n, 8):
        fm.update(torch.from_numpy(X[r0:r0 + 8]).to(cuda_device))
    mu, sigma = fm.finalize()
    want_mean, want_cov = O.mean_cov_longdouble(X)
    sd = np.sqrt(np.diagonal(want_cov).astype(np.float64))
    rel = np.abs((sigma.astype(np.longdouble) - want_cov).astype(np.float64)) / (sd[:, None] * sd[None, :])
    print('offset data: max cov err / sqrt(cov_jj cov_kk) %.3e, max mean err %.3e' % (float(rel.max()), float(np.max(np.abs(mu - want_mean.astype(np.float64))))))
    assert np.all(rel <= 1e-12)
    assert np.all(np.abs((mu.astype(np.longdouble) - want_mean).astype(np.float64)) <= 1e-13)


def test_feature_moments_update_makes_no_device_to_host_copy(cuda_device):
    """50 updates (chunk flushes included) under the profiler: no Memcpy DtoH; the one copy of finalize() is seen, which shows
    that the profiler would have seen others.  The same loop also runs with synchronising calls turned into errors."""
    from torch.profiler import ProfilerActivity, profile
    from inclusivegan_amd import hip_ops
    F = 96
    batches = [torch.randn(8, F, device=cuda_device) for _ in range(50)]
    warm = hip_ops.FeatureMoments(F, cuda_device, chunk_rows=64)
    warm.update(batches[0])
    warm.update(batches[1])
    warm.finalize()
    torch.cuda.synchronize()

    def dtoh(prof):
        return [e.name for e in prof.events() if 'dtoh' in e.name.lower().replace(' ', '') or 'devicetohost' in e.name.lower().replace(' ', '')]

    fm = hip_ops.FeatureMoments(F, cuda_device, chunk_rows=64)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for b in batches:
            fm.update(b)
        torch.cuda.synchronize()
    assert fm.count == 400 and dtoh(prof) == []
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        mu, sigma = fm.finalize()
        torch.cuda.synchronize()
    assert len(dtoh(prof)) == 1, sorted({e.name for e in prof.events()})
    fs = hip_ops.FeatureMoments(F, cuda_device, chunk_rows=64)
    torch.cuda.set_sync_debug_mode('error')
    try:
        for b in batches:
            fs.update(b)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    mu_s, sigma_s = fs.finalize()
    assert mu_s.tobytes() == mu.tobytes() and sigma_s.tobytes() == sigma.tobytes()


# ---- the metric ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def Gs(cuda_device):
    from inclusivegan_amd.dnnlib import tflib
    return tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', num_channels=3,
                         resolution=32, label_size=0, fmap_base=512, device=cuda_device, seed=5)


SYNTHETIC = dict(resolution=32, num_channels=3, label_size=0, data_size=128)
_PROJ = {}


def projection(F, dev):
    if F not in _PROJ:
        _PROJ[F] = torch.randn(3 * 32 * 32, F, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) / 55.0
    return _PROJ[F]


def module_feature_fn(images):
    """A feature network with an importable name: what the on-disk cache of real statistics asks for."""
    module_feature_fn.calls += 1
    f = images.float().reshape(images.shape[0], -1) @ projection(24, images.device)
    module_feature_fn.seen.append(f.cpu().numpy())
    return f


module_feature_fn.calls = 0
module_feature_fn.seen = []


def run_recorded(Gs, num_images, F, convert=lambda f: f, spoil=None, **run):
    """FID.run with a device projection as the feature network -> (metric object, real rows, fake rows as the host saw them)."""
    from inclusivegan_amd.metrics import frechet_inception_distance as FM
    seen = dict(real=[], fake=[], fake_phase=False)

    def feature_fn(images):
        assert images.dtype == torch.uint8 and tuple(images.shape[1:]) == (3, 32, 32)
        f = images.float().reshape(images.shape[0], -1) @ projection(F, images.device)
        if spoil is not None:
            f = spoil(f, seen)
        seen['fake' if seen['fake_phase'] else 'real'].append(f.cpu().numpy())
        return convert(f)

    fid = FM.FID(num_images=num_images, minibatch_per_gpu=32, feature_fn=feature_fn, name='fid%d' % num_images)
    orig = fid._generate
    fid._generate = lambda *a, **k: (seen.__setitem__('fake_phase', True), orig(*a, **k))[1]
    fid.run(Gs, dataset_args=run.pop('dataset_args', SYNTHETIC), mirror_augment=False, log_results=False, **run)
    return fid, np.concatenate(seen['real'])[:num_images], np.concatenate(seen['fake'])[:num_images]


@pytest.mark.parametrize('num_images,F', [(96, 24), (100, 24), (96, 130), (400, 130)])
def test_fid_on_the_device_path(cuda_device, Gs, num_images, F, monkeypatch):
    """The reported value against fid_from_activations on the recorded features, within the project's bar for two evaluations
    of one FID (tests/test_metrics.py: 1e-6 max(1, |want|)); tail minibatch (100, 400 with 32 per batch) and rank-deficient
    covariances (96 < 130) included."""
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.metrics import frechet_inception_distance as FM
    made = []
    orig_init = hip_ops.FeatureMoments.__init__
    monkeypatch.setattr(hip_ops.FeatureMoments, '__init__', lambda self, *a, **k: (made.append(self), orig_init(self, *a, **k))[1])
    fid, real, fake = run_recorded(Gs, num_images, F)
    assert real.shape == fake.shape == (num_images, F)
    assert len(made) == 2 and [m.count for m in made] == [num_images, num_images]           # reals and fakes went through the device path
    want = float(FM.fid_from_activations(real, fake))
    got = float(fid._results[0].value)
    print('FID(%d, %d): device path %.12g host formula %.12g rel %.2e' % (num_images, F, got, want, abs(got - want) / max(1.0, abs(want))))
    assert abs(got - want) <= 1e-6 * max(1.0, abs(want))


def test_fid_host_path_is_unchanged(cuda_device, Gs, monkeypatch):
    from inclusivegan_amd import hip_ops
    from inclusivegan_amd.metrics import frechet_inception_distance as FM

    def no_device_path(*a, **k):
        raise AssertionError('NumPy features must not reach FeatureMoments')

    monkeypatch.setattr(hip_ops, 'FeatureMoments', no_device_path)
    for convert in (lambda f: f.cpu().numpy(), lambda f: f.cpu()):
        fid, real, fake = run_recorded(Gs, 100, 24, convert=convert)
        assert float(fid._results[0].value) == float(FM.fid_from_activations(real, fake))


def test_fid_raises_on_a_non_finite_feature(cuda_device, Gs):
    def spoil(f, seen):
        if seen['fake_phase'] and len(seen['fake']) == 1:
            f = f.clone()
            f[3, 5] = float('nan')
        return f

    with pytest.raises(FloatingPointError, match='1 of the 24 columns of mu of the fake features'):
        run_recorded(Gs, 96, 24, spoil=spoil)


def test_reals_cache_on_disk(cuda_device, Gs, tmp_path, monkeypatch):
    from inclusivegan_amd.metrics import frechet_inception_distance as FM
    from inclusivegan_amd.training import misc, tfrecord
    rng = np.random.RandomState(2)
    os.makedirs(str(tmp_path / 'data' / 'reals'))
    with tfrecord.TFRecordExporter(str(tmp_path / 'data' / 'reals'), 64, print_progress=False) as tfr:
        for _ in range(64):
            tfr.add_image(rng.randint(0, 256, size=(3, 32, 32)).astype(np.uint8))
    monkeypatch.chdir(tmp_path)
    run = dict(dataset_args=dict(tfrecord_dir='reals', resolution=32, max_label_size=0), data_dir=str(tmp_path / 'data'),
               mirror_augment=False, log_results=False)
    module_feature_fn.calls, module_feature_fn.seen = 0, []
    first = FM.FID(num_images=64, minibatch_per_gpu=32, feature_fn=module_feature_fn, name='fid64')
    first.run(Gs, **run)
    assert module_feature_fn.calls == 4                                  # two minibatches of reals, two of fakes
    files = os.listdir(str(tmp_path / '.stylegan2-cache'))
    assert len(files) == 1 and files[0].endswith('-fid64-reals.pkl')
    assert os.path.join('.stylegan2-cache', files[0]) == first._get_cache_file_for_reals(feature_fn=module_feature_fn, num_images=64)
    mu_file, sigma_file = misc.load_pkl(os.path.join('.stylegan2-cache', files[0]))
    assert mu_file.tobytes() == first._real_stats[0].tobytes() and sigma_file.tobytes() == first._real_stats[1].tobytes()
    # a second object reads the file: no real image goes through the feature network
    module_feature_fn.calls, module_feature_fn.seen = 0, []
    second = FM.FID(num_images=64, minibatch_per_gpu=32, feature_fn=module_feature_fn, name='fid64')
    second.run(Gs, **run)
    assert module_feature_fn.calls == 2
    assert second._real_stats[0].tobytes() == mu_file.tobytes() and second._real_stats[1].tobytes() == sigma_file.tobytes()
    want = float(FM.fid_from_statistics(mu_file, sigma_file, *FM.statistics(np.concatenate(module_feature_fn.seen)[:64])))
    assert abs(float(second._results[0].value) - want) <= 1e-6 * max(1.0, abs(want))
    # no importable name, no file
    elsewhere = tmp_path / 'elsewhere'
    elsewhere.mkdir()
    monkeypatch.chdir(elsewhere)
    third = FM.FID(num_images=64, minibatch_per_gpu=32, feature_fn=lambda images: module_feature_fn(images), name='fid64')
    third.run(Gs, **run)
    assert os.listdir(str(elsewhere)) == [] and module_feature_fn.calls == 6
