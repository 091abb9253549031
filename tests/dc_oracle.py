"""fp64 brute force of density and coverage (Naeem et al., ICML 2020; the `prdc` definitions), built on
screening_cases.exact_sqdist, shared by tests/test_density_coverage.py (host) and the two GPU test files.  No device is needed
to import it.

    r2[i, s]    = the value at 0-based position ks[s] of the ascending squared distances of real i to ALL reals, itself included
    count[i, s] = #{ j : d2(real_i, fake_j) < r2[i, s] }          (`<=` with inclusive=True)
    density[s]  = sum_i count[i, s] / (ks[s] * M)                  integer sum, ONE division
    coverage[s] = #{ i : count[i, s] > 0 } / N"""
import numpy as np

from screening_cases import DECIDED_RTOL, exact_sqdist


def radii(reals, ks):
    """-> fp64 [N, len(ks)] squared radii."""
    d2 = exact_sqdist(reals, reals)
    return np.ascontiguousarray(np.sort(d2, axis=1)[:, list(ks)])


def counts(d2_real_fake, r2, inclusive=False):
    """-> int64 [N, nk]."""
    d = d2_real_fake[:, :, None]
    inside = (d <= r2[:, None, :]) if inclusive else (d < r2[:, None, :])
    return inside.sum(axis=1, dtype=np.int64)


def density(count, ks, num_fakes):
    """Python integers up to the one division: -> list of float."""
    return [int(count[:, s].sum()) / (int(k) * int(num_fakes)) for s, k in enumerate(ks)]


def coverage(count):
    return [int((count[:, s] > 0).sum()) / count.shape[0] for s in range(count.shape[1])]


def undecided(d2_real_fake, r2, reals, fakes):
    """The (real, fake, column) triples whose distance neither differs from the real's radius by more than DECIDED_RTOL
    relative nor equals it with bit-identical difference rows (|real - fake| == |real - the real the radius was measured
    to|: then both sides sum the same terms in the same order, whatever that order is, and the tie is exact on the device)."""
    bad = []
    for s in range(r2.shape[1]):
        R = r2[:, s:s + 1]
        near = np.abs(d2_real_fake - R) <= DECIDED_RTOL * np.maximum(d2_real_fake, R)
        for i, j in zip(*np.nonzero(near)):
            ok = False
            if d2_real_fake[i, j] == r2[i, s]:
                own = exact_sqdist(reals[i:i + 1], reals)[0]
                diff = np.abs(reals[i] - fakes[j])
                ok = any(np.array_equal(np.abs(reals[i] - reals[r]), diff) for r in np.nonzero(own == r2[i, s])[0])
            if not ok:
                bad.append((int(i), int(j), s))
    return bad


def assert_decided(d2_real_fake, r2, reals, fakes):
    """A condition on the inputs, asserted on the reference alone: a case that fails it moves to the next seed."""
    bad = undecided(d2_real_fake, r2, reals, fakes)
    assert not bad, 'undecided (real, fake, column): %s' % bad[:4]


def exact_ties(d2_real_fake, r2):
    """How many (real, fake, column) triples sit exactly on a sphere."""
    return int((d2_real_fake[:, :, None] == r2[:, None, :]).sum())


def density_coverage(reals, fakes, ks, inclusive=False):
    """-> dict(radii, d2, counts, density, coverage), the inputs held to the decidedness condition."""
    reals, fakes = np.asarray(reals, np.float32), np.asarray(fakes, np.float32)
    r2 = radii(reals, ks)
    d2 = exact_sqdist(reals, fakes)
    assert_decided(d2, r2, reals, fakes)
    c = counts(d2, r2, inclusive)
    return dict(radii=r2, d2=d2, counts=c, density=density(c, ks, fakes.shape[0]), coverage=coverage(c))
