"""GPU: igan_ball_count_update -- how many candidates lie inside each query's own balls, the count behind density and coverage.

Contract: count[q][s] grows by #{c : d2(q, c) < R[q][s]} (inclusive: <=) on the exact fp64 distance, as integers EQUAL to an
fp64 brute force (tests/dc_oracle.py, tests/screening_cases.py): on the adversarial row families of the screening interval,
where the radii come from the device's own k-th-distance search so that every radius bit-equals one measured distance; at a
dim shorter than a wavefront's stride, with 1 and 8 columns; whatever the candidate batches are and in whatever order they
come; and with the non-finite rows and radii a metric can meet.  One reference per case, shared and never written to."""
import functools

import numpy as np
import pytest
import torch

import dc_oracle
import screening_cases as S

pytestmark = pytest.mark.gpu

NQ, NC, DIM = 70, 136, 768      # the last workgroup has two idle waves; two full strips of candidates and a tail of 8


def device_counts(dev, q, c, radius, inclusive, batches=None):
    """count int64 [nq, nk] after the candidate batches [(begin, end), ...] (default: one batch); radius: fp64 tensor on the device."""
    from inclusivegan_amd import hip_ops
    qd, cd = torch.from_numpy(np.array(q)).to(dev), torch.from_numpy(np.array(c)).to(dev)
    qn, cn = hip_ops.row_sqnorm_raw(qd), hip_ops.row_sqnorm_raw(cd)
    count = hip_ops.ball_count_state(qd.shape[0], radius.shape[1], dev)
    for b, e in batches or [(0, cd.shape[0])]:
        hip_ops.ball_count_update_raw(qd, qn, radius, cd[b:e], cn[b:e], count, inclusive)
    assert count.dtype == torch.int64
    return count.cpu().numpy()


def device_radii(dev, q, c, kcap):
    """The kcap smallest exact squared distances of every query among the candidates, from the device's own search."""
    from inclusivegan_amd import hip_ops
    qd, cd = torch.from_numpy(np.array(q)).to(dev), torch.from_numpy(np.array(c)).to(dev)
    kth = hip_ops.knn_radius_state(qd.shape[0], kcap, dev)
    hip_ops.knn_radius_update_raw(qd, hip_ops.row_sqnorm_raw(qd), cd, hip_ops.row_sqnorm_raw(cd), kth)
    return kth


def expected(d2, srt, inclusive):
    cols = [((d2 <= srt[:, s:s + 1]) if inclusive else (d2 < srt[:, s:s + 1])).sum(1) for s in range(srt.shape[1])]
    return np.stack(cols, axis=1).astype(np.int64)


# ----------------------------------------------------------------------------- adversarial rows
@pytest.mark.parametrize('family', S.FAMILIES)
def test_counts_on_adversarial_rows(cuda_device, family):
    q, c, ans = S.cut(family, NQ, NC, DIM)
    radius = device_radii(cuda_device, q, c, 4)
    got_r = radius.cpu().numpy()
    assert np.all(np.abs(np.sqrt(got_r) - np.sqrt(ans['radius'])) <= 1e-12 * np.sqrt(ans['radius']).max())
    strict, inclusive = expected(ans['d2'], ans['radius'], False), expected(ans['d2'], ans['radius'], True)
    assert np.all(inclusive > strict)           # every radius IS a distance of its row: the two comparisons differ on every entry
    if family == 'flat_u8':                     # uint8 levels tie in droves: the strict count stays below s, the inclusive one jumps
        assert (inclusive - strict).max() >= 4 and (strict[:, 3] < 3).mean() > 0.5 and inclusive[:, 3].min() == 4
    got_strict = device_counts(cuda_device, q, c, radius, False)
    got_inclusive = device_counts(cuda_device, q, c, radius, True)
    print('%-10s strict column sums %s inclusive %s' % (family, got_strict.sum(0).tolist(), got_inclusive.sum(0).tolist()))
    assert np.array_equal(got_strict, strict)
    assert np.array_equal(got_inclusive, inclusive)


# ----------------------------------------------------------------------------- other shapes
def clustered_sets(dim, n_real, n_fake, seed):
    """Clustered reals, and fakes partly near them and partly far: both small and large counts occur."""
    rng = np.random.RandomState(seed)
    centres = rng.randn(12, dim)
    real = (centres[rng.randint(0, 12, size=n_real)] + 0.3 * rng.randn(n_real, dim)).astype(np.float32)
    near = real[rng.randint(0, n_real, size=n_fake // 2)] + (0.25 * rng.randn(n_fake // 2, dim)).astype(np.float32)
    far = (1.5 * rng.randn(n_fake - n_fake // 2, dim)).astype(np.float32)
    return real, np.concatenate([near, far]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def dim50_case():
    """333 x 301 at dim 50: a row is shorter than the 64 floats a wavefront strides over.  The radii are those of the reals
    among themselves at k = 1 .. 8 (the metric's orientation); held to the decidedness condition."""
    real, fake = clustered_sets(50, 333, 301, seed=50)
    ks = list(range(1, 9))
    ref = {inc: dc_oracle.density_coverage(real, fake, ks, inclusive=inc) for inc in (False, True)}
    for r in ref.values():
        for a in (r['radii'], r['d2'], r['counts']):
            a.setflags(write=False)
    return real, fake, ref


@pytest.mark.parametrize('columns', [[4], list(range(8))])
def test_real_valued_rows_at_dim_50_with_1_and_8_columns(cuda_device, columns):
    real, fake, ref = dim50_case()
    radius = device_radii(cuda_device, real, real, 9)[:, 1:][:, columns].contiguous()        # k = 1 .. 8 are positions 1 .. 8
    want_r = ref[False]['radii'][:, columns]
    assert np.all(np.abs(radius.cpu().numpy() - want_r) <= 1e-11 * want_r)
    for inclusive in (False, True):
        got = device_counts(cuda_device, real, fake, radius, inclusive)
        want = ref[inclusive]['counts'][:, columns]
        assert got.shape == (333, len(columns)) and np.array_equal(got, want)
        assert 0 < (want > 0).mean() < 1 and want.max() > 1


# ----------------------------------------------------------------------------- batching
def test_batches_and_their_order_do_not_matter(cuda_device):
    q, c, ans = S.cut('flat_noisy', NQ, NC, DIM)
    radius = device_radii(cuda_device, q, c, 4)
    whole = device_counts(cuda_device, q, c, radius, False)
    assert np.array_equal(whole, expected(ans['d2'], ans['radius'], False))
    for step in (50, 64, 136):
        batches = [(b, min(b + step, NC)) for b in range(0, NC, step)]
        for order in (batches, batches[::-1]):
            assert device_counts(cuda_device, q, c, radius, False, order).tobytes() == whole.tobytes(), (step, order[0])
    # no early exit and no saturation: a batch fed twice counts twice
    twice = device_counts(cuda_device, q, c, radius, False, [(0, NC), (0, NC)])
    assert np.array_equal(twice, 2 * whole) and whole.sum() > 0
    one = device_counts(cuda_device, q, c, radius, True, [(0, 50), (0, 50), (50, NC)])
    assert np.array_equal(one, expected(ans['d2'], ans['radius'], True) + expected(ans['d2'][:, :50], ans['radius'], True))


# ----------------------------------------------------------------------------- special values
def test_non_finite_rows_and_radii(cuda_device):
    dev = cuda_device
    rng = np.random.RandomState(8)
    q = rng.randn(6, 40).astype(np.float32)
    c = (rng.randn(70, 40) * 1.05).astype(np.float32)
    c[10] = q[2]
    c[20] = q[2]                                # two exact copies of query 2
    c[3, 5] = np.nan                            # a NaN candidate row
    c[66, 7] = np.inf                           # a +inf candidate row
    q[4, 1] = np.nan                            # a NaN query row
    clean = np.delete(c, [3, 66], axis=0)
    d2 = S.exact_sqdist(q, clean)
    srt = np.sort(np.where(np.isnan(d2), np.inf, d2), axis=1)
    R = (0.5 * srt[:, 6] + 0.5 * srt[:, 7])[:, None]           # between the 7th and the 8th smallest distance of a row: no pair is near it
    columns = np.concatenate([R, np.full_like(R, np.inf), np.zeros_like(R), np.full_like(R, np.nan), np.full_like(R, -1.0)], axis=1)
    assert not dc_oracle.undecided(np.delete(d2, 4, axis=0), np.delete(R, 4, axis=0), np.delete(q, 4, axis=0), clean)
    radius = torch.from_numpy(columns).to(dev)
    ok = np.arange(6) != 4
    for inclusive in (False, True):
        got = device_counts(dev, q, c, radius, inclusive)
        with np.errstate(invalid='ignore'):
            want = dc_oracle.counts(d2, columns, inclusive)
        # the NaN and +inf candidates are never counted and change no other count: the counts are those of the clean candidates
        assert np.array_equal(got[ok], want[ok]), inclusive
        assert np.array_equal(got[ok, 0], np.full(5, 7))
        assert np.array_equal(got[4], np.zeros(5))                          # a NaN query counts nothing, whatever the radius
        assert np.array_equal(got[ok, 1], np.full(5, 68))                   # radius +inf: every candidate at a finite distance
        assert np.array_equal(got[ok, 2], [0, 0, 2, 0, 0] if inclusive else [0] * 5)      # radius 0: exact copies, and only inclusively
        assert np.array_equal(got[:, 3], np.zeros(6)) and np.array_equal(got[:, 4], np.zeros(6))       # NaN, negative radius
    # every radius column at once, in candidate batches that cut between the special rows
    parts = device_counts(dev, q, c, radius, False, [(0, 5), (5, 66), (66, 70)])
    assert np.array_equal(parts, device_counts(dev, q, c, radius, False))


def test_overflowing_products_are_measured(cuda_device):
    """Rows of 3e19: the fp32 norms and products overflow, the screening interval is NaN and decides nothing, so the pair is
    measured -- the exact distance of two identical rows is 0, inside any positive radius and on a sphere of radius 0."""
    dev = cuda_device
    rng = np.random.RandomState(9)
    q = rng.randn(3, 96).astype(np.float32)
    c = rng.randn(66, 96).astype(np.float32)
    q[1] = 3e19
    c[65] = 3e19
    c[7] = 3e19
    c[7, 0] = -3e19                                  # differs in one element: (6e19)^2 away, finite in fp64
    d2 = S.exact_sqdist(q, c)
    assert d2[1, 65] == 0 and np.isfinite(d2).all() and 3e39 < d2[1, 7] < 4e39 and np.delete(d2[1], [7, 65]).min() > 1e40
    columns = np.array([[1.0, 0.0, 1e40, np.inf]] * 3)
    radius = torch.from_numpy(columns).to(dev)
    for inclusive in (False, True):
        got = device_counts(dev, q, c, radius, inclusive)
        assert np.array_equal(got, dc_oracle.counts(d2, columns, inclusive)), inclusive
        assert got[1].tolist() == [1, 1 if inclusive else 0, 2, 66]


# ----------------------------------------------------------------------------- wrapper
def test_wrapper_rejects_what_the_entry_cannot_take(cuda_device):
    from inclusivegan_amd import hip_ops
    dev = cuda_device
    q, c = torch.zeros(8, 16, device=dev), torch.zeros(6, 16, device=dev)
    qn, cn = torch.zeros(8, device=dev), torch.zeros(6, device=dev)
    rad = torch.ones(8, 2, device=dev, dtype=torch.float64)
    count = hip_ops.ball_count_state(8, 2, dev)
    hip_ops.ball_count_update_raw(q, qn, rad, c, cn, count)
    assert count.cpu().tolist() == [[6, 6]] * 8                      # distance 0 < 1 for every pair
    hip_ops.ball_count_update_raw(q[2:5], qn[2:5], rad[2:5], c, cn, count[2:5], inclusive=True)      # a contiguous row view is a state
    assert count.cpu().tolist() == [[6, 6]] * 2 + [[12, 12]] * 3 + [[6, 6]] * 3
    with pytest.raises(TypeError):
        hip_ops.ball_count_update_raw(q, qn, rad.float(), c, cn, count)
    with pytest.raises(TypeError):
        hip_ops.ball_count_update_raw(q, qn, rad.cpu(), c, cn, count)
    with pytest.raises(TypeError):
        hip_ops.ball_count_update_raw(q, qn, rad, c, cn, count.int())
    with pytest.raises(TypeError):
        hip_ops.ball_count_update_raw(q, qn, rad, c, cn, count[:, :1])              # not contiguous
    with pytest.raises(TypeError):
        hip_ops.ball_count_update_raw(q, qn, rad, c, cn, count[:, 0])               # one dimension
    with pytest.raises(ValueError):
        hip_ops.ball_count_update_raw(q, qn, rad, c, cn, count[:7])                 # one row per query
    with pytest.raises(ValueError):
        hip_ops.ball_count_update_raw(q, qn, rad[:, :1], c, cn, count)              # nk of radius and count
    with pytest.raises(ValueError):
        hip_ops.ball_count_update_raw(q, qn, rad, c[:, :8], cn, count)              # dims
    with pytest.raises(ValueError):
        hip_ops.ball_count_update_raw(q, qn[:7], rad, c, cn, count)
    with pytest.raises(ValueError):
        hip_ops.ball_count_update_raw(q, qn, rad, c, cn[:5], count)
    with pytest.raises(ValueError):
        hip_ops.ball_count_state(8, 9, dev)
