"""Row families that are adversarial for the screening interval of the exact searches (csrc/exact_distance.h), their fp64
brute force and the interval arithmetic restated, shared by tests/test_screening_cases.py (host) and
tests/test_gpu_screening.py.  No device is needed to import it.

Every exact search (exact_search.hip, kmeans.hip) forms a = |q|^2 + |c|^2 - 2 q.c from an fp32 product and
measures a pair in fp64 only when [a - t, a + t], t = nn1_tol(dim) * (|q|^2 + |c|^2), cannot decide it.  That is sound only
while |a - d2_exact| <= t; interval_use() is the ratio rho of the two, per pair.  On rows whose products all have one sign and
one size (flat images) the rounding errors of a running fp32 sum do not cancel: they grow like dim, not like sqrt(dim).

A case is a seeded (q [nq, dim], c [nc, dim]) fp32 pair.  Candidate rows 1 and 2 are an exact duplicate pair placed next to
query 0 (the lower-index rule); in the flat families rows 3 .. 3 + 8 P are planted next to the first P = min(nq, nc // 16)
queries, 8 each (slot s belongs to query (s - 3) % P), so that every prefix c[:n] of a case keeps near-ties.  The GPU tests cut
their shapes out of one case per (family, dim): q[:nq], c[:nc]."""
import functools

import numpy as np

FAMILIES = ('zero_mean', 'positive', 'offset', 'anti', 'spiky', 'flat', 'flat_u8', 'flat_noisy')
PLANTED_PER_QUERY = 8
K_NEIGHBOURS = 10       # the k smallest pairs the brute force keeps
K_RADIUS = 3            # the radius of a row is its 3rd-smallest distance (pr50k3)
DECIDED_RTOL = 1e-9     # consecutive distinct exact distances differ by more than this: four orders above the ~1e-13 by which two fp64 summation orders differ
U32 = 2.0 ** -24        # unit roundoff of fp32


def nn1_tol(dim):
    """csrc/exact_distance.h, `nn1_tol`: (dim + 2) u / (1 - (dim + 2) u), u = 2^-24 -- a bound for any order of `dim` roundings.
    Stated once in Python, by hip_ops.screening_tol (tests/test_exact_search.py holds it to the closed form)."""
    from inclusivegan_amd import hip_ops
    return hip_ops.screening_tol(dim)


def statistical_tol(dim):
    """max(2^-22 sqrt(dim), 1e-6): the interval nn1_tol was before -- the rounding errors of the chain taken for a random walk.
    Kept to show that the cases discriminate: flat rows leave it, random rows do not."""
    return max(2.0 ** -22 * np.sqrt(float(dim)), 1e-6)


def _u8_level(code):
    """training/misc.py adjust_dynamic_range([0, 255] -> [-1, 1]) on a uint8 code: fp32 scale and bias, one rounding each."""
    scale = (np.float32(1) - np.float32(-1)) / (np.float32(255) - np.float32(0))
    bias = np.float32(-1) - np.float32(0) * scale
    return (np.asarray(code, np.float32) * scale + bias).astype(np.float32)


def _flat(levels, dim):
    return np.repeat(np.asarray(levels, np.float32)[:, None], dim, axis=1)


def make(name, nq, nc, dim, seed):
    """One (q, c) pair of family `name`, contiguous fp32."""
    assert name in FAMILIES and nc >= 3 and dim >= 2
    rng = np.random.RandomState(seed)
    P = min(nq, nc // 16)
    slots = np.arange(3, 3 + PLANTED_PER_QUERY * P)
    owner = (slots - 3) % max(P, 1)
    if name in ('flat', 'flat_u8'):
        if name == 'flat':
            ql = rng.uniform(0.2, 0.9, size=nq)
            cl = rng.uniform(0.2, 0.9, size=nc)
            cl[slots] = ql[owner] + rng.uniform(-2e-3, 2e-3, size=slots.size)
            cl[1] = cl[2] = ql[0] + 1e-3
            ql, cl = ql.astype(np.float32), cl.astype(np.float32)
        else:
            qk = rng.randint(1, 255, size=nq)
            ck = rng.randint(0, 256, size=nc)
            ck[slots] = qk[owner] + rng.randint(-1, 2, size=slots.size)
            ck[1] = ck[2] = qk[0]
            ql, cl = _u8_level(qk), _u8_level(ck)
        return _flat(ql, dim), _flat(cl, dim)
    if name == 'zero_mean':
        q, c, bump = rng.uniform(-1, 1, size=(nq, dim)), rng.uniform(-1, 1, size=(nc, dim)), 0.25
    elif name == 'positive':
        q, c, bump = rng.uniform(0.5, 1, size=(nq, dim)), rng.uniform(0.5, 1, size=(nc, dim)), 0.125
    elif name == 'offset':
        q, c, bump = 100 + 1e-2 * rng.randn(nq, dim), 100 + 1e-2 * rng.randn(nc, dim), 0.25
    elif name == 'anti':
        q = rng.uniform(-1, 1, size=(nq, dim))
        c, bump = -q[np.arange(nc) % nq] + 1e-3 * rng.randn(nc, dim), 0.25
    elif name == 'spiky':
        q, c, bump = 1e-3 * rng.randn(nq, dim), 1e-3 * rng.randn(nc, dim), 1e-3
        q[:, :dim // 64] = 1e3
        c[:, :dim // 64] = 1e3
    else:       # flat_noisy
        q = rng.uniform(0.2, 0.9, size=(nq, 1)) + 1e-3 * rng.randn(nq, dim)
        c, bump = rng.uniform(0.2, 0.9, size=(nc, 1)) + 1e-3 * rng.randn(nc, dim), 1e-3
    q, c = q.astype(np.float32), c.astype(np.float32)
    c[1] = q[0]
    c[1, dim - 1] += np.float32(bump)       # next to query 0 ...
    c[2] = c[1]                             # ... and its exact duplicate
    return np.ascontiguousarray(q), np.ascontiguousarray(c)


def exact_sqdist(q, c):
    """d2[i, j] = sum (q[i] - c[j])^2: direct differences of the fp32 rows, summed in fp64 (prd_oracle.sqdist, imle_cases.exact_knn)."""
    q = np.asarray(q, np.float64)
    c = np.asarray(c, np.float64)
    out = np.empty((q.shape[0], c.shape[0]), np.float64)
    d = np.empty_like(c)
    for i in range(q.shape[0]):
        np.subtract(c, q[i], out=d)
        out[i] = np.einsum('ij,ij->i', d, d)
    return out


def undecided(d2, q, c, top):
    """The decidedness condition on the `top` smallest distances of every row of d2: consecutive values differ by more than
    DECIDED_RTOL relative, or are EQUAL with bit-identical difference rows |q - c| (then both sides sum the same terms in the
    same order, whatever that order is: the tie is exact on the device too and goes to the lower index).  Bit-identical
    candidate rows are the usual such pair; flat uint8 levels one code either side of a query are the other.
    -> list of offending (query, candidate, candidate) triples: empty when the case is decided."""
    bad = []
    for i in range(d2.shape[0]):
        o = np.argsort(d2[i], kind='stable')[:top]
        for a, b in zip(o[:-1], o[1:]):
            da, db = d2[i, a], d2[i, b]
            if da == db:
                if not np.array_equal(np.abs(q[i] - c[a]), np.abs(q[i] - c[b])):
                    bad.append((i, int(a), int(b)))
            elif not (db - da) > DECIDED_RTOL * db:
                bad.append((i, int(a), int(b)))
    return bad


def brute(q, c, d2=None, centres=20):
    """The answers every consumer must reproduce, all from ONE exact distance matrix; ties go to the lower index.
      nn_idx [nq]                 nearest candidate
      knn_idx, knn_d2 [nq, k]     the k = min(10, nc) smallest (distance, index) pairs
      radius [nq, 4]              the 4 smallest distances of a query among the candidates (kcap 4; column 2 is the radius)
      cand_radius [nc, 3]         the 3 smallest distances of a candidate among the queries
      member [nq, 3]              per column s: some candidate has the query within ITS radius cand_radius[c, s] (`<=`)
      label, label_d2 [nq]        nearest of the first `centres` candidates (the k-means step's centres)"""
    if d2 is None:
        d2 = exact_sqdist(q, c)
    nq, nc = d2.shape
    k = min(K_NEIGHBOURS, nc)
    order = np.argsort(d2, axis=1, kind='stable')
    knn_idx = order[:, :k].astype(np.int32)
    srt = np.take_along_axis(d2, order, axis=1)
    cand_radius = np.ascontiguousarray(np.sort(d2, axis=0)[:K_RADIUS].T)
    member = np.stack([(d2 <= cand_radius[None, :, s]).any(axis=1) for s in range(cand_radius.shape[1])], axis=1)
    nk = min(centres, nc)
    label = np.argmin(d2[:, :nk], axis=1).astype(np.int32)
    return dict(d2=d2, nn_idx=knn_idx[:, 0].copy(), knn_idx=knn_idx, knn_d2=srt[:, :k].copy(), radius=srt[:, :K_RADIUS + 1].copy(),
                cand_radius=cand_radius, member=member, label=label,
                label_d2=d2[np.arange(nq), label])


def assert_decided(q, c, d2):
    """Asserted when a case is built, and on every cut of it a test uses: the 11 smallest per query (the k = 10 pairs and the one
    behind them), and the 4 smallest per candidate among the queries (the radius and its two neighbours)."""
    bad = undecided(d2, q, c, K_NEIGHBOURS + 1)
    assert not bad, 'undecided neighbours (query, candidate, candidate): %s' % bad[:4]
    bad = undecided(d2.T, c, q, K_RADIUS + 1)
    assert not bad, 'undecided radii (candidate, query, query): %s' % bad[:4]
    # the duplicate pair is among query 0's k smallest, the copy right behind the original
    o = np.argsort(d2[0], kind='stable')[:K_NEIGHBOURS].tolist()
    assert np.array_equal(c[1], c[2]) and d2[0, 1] == d2[0, 2] and 1 in o[:-1] and o[o.index(1) + 1] == 2, o


# A seed is the family's number and the dim; where the reference alone did not meet the decidedness condition at that seed the
# case moved to the next one, listed here (a condition on the inputs, never a measurement of the code under test).
RESEED = {}


@functools.lru_cache(maxsize=None)
def case(name, nq, nc, dim):
    """-> (q, c, answers of brute()), decided; cached and shared: never written to."""
    seed = 7000 + 100 * FAMILIES.index(name) + dim % 97 + RESEED.get((name, nq, nc, dim), 0)
    q, c = make(name, nq, nc, dim, seed)
    ans = brute(q, c)
    assert_decided(q, c, ans['d2'])
    for a in (q, c) + tuple(ans.values()):
        a.setflags(write=False)
    return q, c, ans


def cases(nq, nc, dim):
    """{family: (q, c)} for every family at one shape."""
    return {name: case(name, nq, nc, dim)[:2] for name in FAMILIES}


def cut(name, nq, nc, dim, base=(72, 136)):
    """q[:nq], c[:nc] of the family's one case at `dim` and the brute-force answers of the cut (its distance block is a block
    of the case's: the reference is computed once per (family, dim)); the cut is held to the decidedness condition itself."""
    q, c, ans = case(name, base[0], base[1], dim)
    assert nq <= base[0] and nc <= base[1]
    q, c = q[:nq], c[:nc]
    sub = brute(q, c, d2=np.ascontiguousarray(ans['d2'][:nq, :nc]))
    assert_decided(q, c, sub['d2'])
    return q, c, sub


def row_sqnorm32(a):
    """igan_row_sqnorm: an fp64 sum of squares, rounded to fp32."""
    a = np.asarray(a, np.float64)
    return np.einsum('ij,ij->i', a, a).astype(np.float32)


def interval_use(q, c, dots, qnorm, cnorm, d2=None, tol=nn1_tol):
    """rho[i, j] = |a - d2_exact| / t with a = qn + cn - 2 dot and t = nn1_tol(dim) * (qn + cn), in fp64 on the fp32 values the
    kernels read, exactly as the fold kernels form them (exact_search.h, screen_interval).  rho <= 1 is what the screen needs."""
    if d2 is None:
        d2 = exact_sqdist(q, c)
    qn = np.asarray(qnorm, np.float32).astype(np.float64)[:, None]
    cn = np.asarray(cnorm, np.float32).astype(np.float64)[None, :]
    a = qn + cn - 2.0 * np.asarray(dots, np.float32).astype(np.float64)
    t = tol(q.shape[1]) * (qn + cn)
    return np.abs(a - d2) / t


def chain_dots(q, c, n):
    """Host model of ONE fp32 accumulator over the whole reduction: fp32 products, groups of n consecutive products summed
    exactly, a strictly sequential running sum with one fp32 rounding per group -- for n = 1 np.cumsum(products, dtype=float32)'s
    last column.  n = 2 is the shape of v_mfma_f32_32x32x2_f32 (two products per accumulate)."""
    q = np.asarray(q, np.float32)
    c = np.asarray(c, np.float32)
    dim = q.shape[1]
    assert dim % n == 0
    s = np.zeros((q.shape[0], c.shape[0]), np.float32)
    ct = np.ascontiguousarray(c.T)
    for k0 in range(0, dim, n):
        g = np.zeros(s.shape, np.float64)
        for k in range(k0, k0 + n):
            g += np.multiply.outer(q[:, k], ct[k]).astype(np.float64)      # the fp32 product, held in fp64
        s = (s.astype(np.float64) + g).astype(np.float32)
    return s


def modelled_screen_keeps(q, c, dots, qnorm, cnorm, tol=nn1_tol):
    """The 1-NN screen of exact_search.hip on given products: the smallest upper bound a + t, then every candidate whose lower bound
    a - t exceeds it is dropped.  -> bool [nq, nc], True where a candidate is still measured."""
    qn = np.asarray(qnorm, np.float32).astype(np.float64)[:, None]
    cn = np.asarray(cnorm, np.float32).astype(np.float64)[None, :]
    a = qn + cn - 2.0 * np.asarray(dots, np.float32).astype(np.float64)
    t = tol(q.shape[1]) * (qn + cn)
    u = (a + t).min(axis=1, keepdims=True)
    return (a - t) <= u
