"""Golden values of k-NN precision / recall, produced by EXECUTING the reference's own ManifoldEstimator.

metrics/precision_recall.py imports TensorFlow at module level and cannot be imported here, but its `ManifoldEstimator`
class (:61-134) is plain NumPy on top of a distance block.  This script parses the reference file where it lies
(/root/reference; nothing is copied), takes the class node, executes it with only `np` in its namespace and hands it a
NumPy fp64 distance block in the reference's clamped form, maximum(|u|^2 - 2 u v^T + |v|^2, 0) (:32).  It is run both ways
on seeded inputs: the manifold of the reference set evaluated on the other set with realism and neighbours (precision,
:157) and the reverse (recall, :161).

The reference stores distances and radii in float16, so the inputs are chosen to make that lossless: integer-valued
features whose squared distances are integers <= 2048.  The script asserts that, and that the executed reference equals
its own fp64 brute force in radii, predictions and nearest indices.  The realism score is a quotient: the reference's is
the float16 one; the fixture stores the float32 value of the fp64 quotient and the script asserts that it rounds to the
reference's float16 value (inf / nan in the same places).
Each case mixes perturbed copies of reference rows with uniform draws, holds one exact copy and one duplicated reference
row, and has many pairs sitting exactly on a radius (`<=` and the position rule with ties are exercised).
Output: tests/golden/pr_golden.npz.  Run: python tests/golden/make_pr_golden.py"""
import ast
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/metrics/precision_recall.py'

# name: (dim, coordinate range, reference points, evaluated points, share of uniform draws among the evaluated, nhood sizes)
CASES = dict(
    a=(64, 2, 257, 300, 0.25, [3]),
    b=(32, 3, 700, 500, 0.30, [3, 5]),
    c=(128, 1, 400, 400, 0.55, [3]),
)


def reference_class():
    mod = ast.parse(open(REF).read())
    node = [n for n in mod.body if isinstance(n, ast.ClassDef) and n.name == 'ManifoldEstimator'][0]
    m = ast.Module(body=[node], type_ignores=[])
    ast.fix_missing_locations(m)
    ns = dict(np=np)
    exec(compile(m, '<reference ManifoldEstimator>', 'exec'), ns)
    return ns['ManifoldEstimator']


class Fp64DistanceBlock:
    def pairwise_distances(self, U, V):
        U = np.asarray(U, np.float64)
        V = np.asarray(V, np.float64)
        return np.maximum((U * U).sum(1)[:, None] - 2.0 * U @ V.T + (V * V).sum(1)[None, :], 0.0)


def sqdist(A, B):
    """Direct-difference squared distances in fp64 (exact: the features are small integers)."""
    out = np.empty((A.shape[0], B.shape[0]), np.float64)
    for i in range(0, A.shape[0], 64):
        d = A[i:i + 64, None, :].astype(np.float64) - B[None, :, :].astype(np.float64)
        out[i:i + 64] = (d * d).sum(2)
    return out


def brute(ref, ev, nhood):
    radii = np.sort(sqdist(ref, ref), axis=1)[:, nhood]
    d = sqdist(ev, ref)
    pred = (d[:, :, None] <= radii[None, :, :]).any(axis=1).astype(np.int32)
    nearest = np.argmin(d, axis=1).astype(np.int32)
    with np.errstate(divide='ignore', invalid='ignore'):
        realism = (radii[nearest, 0] / d.min(axis=1)).astype(np.float32)
    on_radius = int((d[:, :, None] == radii[None, :, :]).sum())
    return radii, pred, nearest, realism, on_radius, float(d.max())


def make_features(rng, dim, r, n_ref, n_eval, uniform_share):
    # reference rows: corners of the cube in groups of about twenty, a few coordinates of each row pulled in
    base = rng.choice([-r, r], size=(max(4, n_ref // 20), dim))
    group = rng.randint(0, base.shape[0], size=n_ref)
    ref = base[group].copy()
    pull = rng.rand(n_ref, dim) < 0.08
    ref[pull] -= np.sign(ref[pull]) * rng.randint(1, r + 1, size=int(pull.sum()))
    ref[1] = ref[0]                                        # a duplicated reference row
    n_uni = int(round(uniform_share * n_eval))
    covered = np.flatnonzero(group < (base.shape[0] + 1) // 2)  # perturbed copies of half the groups only: the rest is not covered
    src = covered[rng.randint(0, covered.shape[0], size=n_eval - n_uni)]
    near = ref[src].copy()
    flip = rng.rand(*near.shape) < 0.1
    near[flip] = np.clip(near[flip] + rng.choice([-1, 1], size=int(flip.sum())), -r, r)
    near[0] = ref[src[0]]                                  # an exact copy
    uni = rng.randint(-r, r + 1, size=(n_uni, dim))
    ev = np.concatenate([near, uni])[rng.permutation(n_eval)]
    return ref.astype(np.int8), ev.astype(np.int8)


def main():
    Ref = reference_class()
    rng = np.random.RandomState(20240607)
    out = {}
    in_band = 0
    for name, (dim, r, n_ref, n_eval, share, nhood) in CASES.items():
        ref, ev = make_features(rng, dim, r, n_ref, n_eval, share)
        assert ref.shape == (n_ref, dim) and ev.shape == (n_eval, dim)
        f_ref, f_ev = ref.astype(np.float32), ev.astype(np.float32)
        block = Fp64DistanceBlock()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                 # the reference divides by a zero distance at the exact copy
            m_ref = Ref(block, f_ref, 100, 128, nhood)
            m_ev = Ref(block, f_ev, 37, 61, nhood)
            precision, realism, nearest = m_ref.evaluate(f_ev, return_realism=True, return_neighbors=True)
            recall = m_ev.evaluate(f_ref)
        b_rad, b_prec, b_near, b_real, ties_p, dmax_p = brute(ref, ev, nhood)
        e_rad, b_rec, _, _, ties_r, dmax_r = brute(ev, ref, nhood)
        dmax = max(dmax_p, dmax_r, float(sqdist(ref, ref).max()), float(sqdist(ev, ev).max()))
        assert dmax <= 2048, dmax
        # the executed reference equals the fp64 brute force
        assert m_ref.D.dtype == np.float16 and np.array_equal(m_ref.D.astype(np.float64), b_rad)
        assert np.array_equal(m_ev.D.astype(np.float64), e_rad)
        assert precision.dtype == np.int32 and np.array_equal(precision, b_prec) and np.array_equal(recall, b_rec)
        assert nearest.dtype == np.int32 and np.array_equal(nearest, b_near)
        assert realism.dtype == np.float32
        finite = np.isfinite(b_real)
        assert np.array_equal(np.isnan(realism), np.isnan(b_real)) and np.array_equal(np.isinf(realism), np.isinf(b_real))
        assert np.array_equal(b_real[finite].astype(np.float16), realism[finite].astype(np.float16))
        assert np.isinf(b_real).sum() >= 1 and ties_p > 0 and ties_r > 0
        kp, kr = precision.mean(axis=0), recall.mean(axis=0)
        in_band += bool(np.all((kp > 0.2) & (kp < 0.8) & (kr > 0.2) & (kr < 0.8)))
        print('%s: dim %d ref %d eval %d nhood %s  precision %s recall %s  max d2 %d  pairs on a radius %d / %d  inf realism %d'
              % (name, dim, n_ref, n_eval, nhood, kp, kr, dmax, ties_p, ties_r, int(np.isinf(b_real).sum())))
        out['%s/ref' % name] = ref; out['%s/eval' % name] = ev
        out['%s/nhood_sizes' % name] = np.asarray(nhood, np.int32)
        out['%s/ref_radii' % name] = b_rad; out['%s/eval_radii' % name] = e_rad
        out['%s/precision' % name] = precision; out['%s/recall' % name] = recall
        out['%s/realism' % name] = b_real; out['%s/nearest' % name] = nearest
        out['%s/knn_precision' % name] = kp.astype(np.float64); out['%s/knn_recall' % name] = kr.astype(np.float64)
    assert in_band >= 1, 'no case has both means inside (0.2, 0.8)'
    out['cases'] = np.asarray(sorted(CASES))
    np.savez_compressed(os.path.join(HERE, 'pr_golden.npz'), **out)


if __name__ == '__main__':
    main()
