"""Golden values for linear separability (ls) and the Inception Score (is50k), produced by EXECUTING the reference's own
statements and by sklearn's LinearSVC, the reference's solver.  Results only: the inputs are regenerated from seeds
(tests/ls_cases.py and the generators below).

  information functions   prob_normalize / mutual_information / entropy / conditional_entropy are cut out of
                          /root/reference/metrics/linear_separability.py (the file imports TensorFlow and sklearn at module
                          level; nothing is copied) and run on seeded 2x2 tables, tables with zero cells and the
                          perfect-prediction table among them;
  IS                      the statements after the sampling loop of IS._evaluate (:49-56) on seeded probabilities with a split
                          count that does not divide n;
  per case of ls_cases    W_tight: LinearSVC(dual=False, tol=1e-12, max_iter=100000) per attribute on its kept rows;
                          d_ref: the relative L2 distance of LinearSVC() AT ITS DEFAULTS (the reference's call, :162) from
                          W_tight over the solved attributes, for dual=True and dual=False -- how far the reference's own
                          call stays from the minimiser; the confusion tables (:170) and conditional entropies of W_tight's
                          predictions.
Output: tests/golden/ls_golden.npz.  Run: python tests/golden/make_ls_golden.py"""
import ast
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ls_cases  # noqa: E402

REF = '/root/reference/metrics'


def info_tables():
    rng = np.random.RandomState(7)
    tables = [rng.randint(1, 1000, size=(2, 2)).astype(np.float64) for _ in range(6)]
    tables += [rng.rand(2, 2) for _ in range(4)]
    tables += [np.array([[0.37, 0.0], [0.0, 0.63]]), np.array([[0.5, 0.0], [0.0, 0.5]]), np.array([[1.0, 0.0], [0.0, 0.0]]),
               np.array([[0.2, 0.3], [0.0, 0.5]]), np.array([[0.0, 0.4], [0.6, 0.0]]), np.array([[0.25, 0.25], [0.25, 0.25]])]
    return np.stack(tables)


def is_probabilities():
    rng = np.random.RandomState(11)
    logits = 2.0 * rng.randn(103, 17)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32), 7        # 7 does not divide 103


def reference_info_functions():
    mod = ast.parse(open(os.path.join(REF, 'linear_separability.py')).read())
    names = ('prob_normalize', 'mutual_information', 'entropy', 'conditional_entropy')
    fns = [n for n in mod.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(fns) == 4
    ns = {'np': np}
    exec(compile(ast.fix_missing_locations(ast.Module(body=fns, type_ignores=[])), '<reference statements>', 'exec'), ns)
    return ns


class Recorder:
    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.values = []

    def _report_result(self, value, suffix='', fmt=''):
        self.values.append((suffix, value))


def reference_is_tail(activations, num_splits):
    mod = ast.parse(open(os.path.join(REF, 'inception_score.py')).read())
    cls = [n for n in mod.body if isinstance(n, ast.ClassDef) and n.name == 'IS'][0]
    body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == '_evaluate'][0].body
    tail = body[-4:]            # scores = [], the loop over the splits, the two reports
    assert isinstance(tail[0], ast.Assign) and tail[0].targets[0].id == 'scores' and isinstance(tail[1], ast.For)
    rec = Recorder(num_images=activations.shape[0], num_splits=num_splits)
    ns = {'np': np, 'self': rec, 'activations': activations}
    exec(compile(ast.fix_missing_locations(ast.Module(body=tail, type_ignores=[])), '<reference statements>', 'exec'), ns)
    return np.asarray(ns['scores']), dict(rec.values)


def svc_weights(X, Y, **kw):
    import sklearn.svm          # only the generator needs it: the tests import this module for its seeded inputs
    W = np.zeros((Y.shape[1], X.shape[1] + 1))
    for a in range(Y.shape[1]):
        rows = Y[:, a] != 0
        y = Y[rows, a]
        if (y > 0).any() and (y < 0).any():
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')       # the dual solver's ConvergenceWarning is the point of d_ref
                svm = sklearn.svm.LinearSVC(**kw).fit(X[rows], y)
            W[a, :-1], W[a, -1] = svm.coef_[0], svm.intercept_[0]
    return W


def main():
    out = {}
    ref = reference_info_functions()
    tables = info_tables()
    for fn in ('mutual_information', 'entropy', 'conditional_entropy'):
        out['info_' + fn] = np.array([ref[fn](t) for t in tables], dtype=np.float64)
    out['info_prob_normalize'] = np.stack([ref['prob_normalize'](t) for t in tables])

    probs, splits = is_probabilities()
    scores, reported = reference_is_tail(probs, splits)
    out['is_scores'] = scores.astype(np.float64)
    out['is_mean'], out['is_std'] = np.float64(reported['_mean']), np.float64(reported['_std'])

    for name in ls_cases.SHAPES:
        X, Y = ls_cases.make_case(name)
        tight = svc_weights(X, Y, dual=False, tol=1e-12, max_iter=100000)
        solved = np.abs(tight).sum(axis=1) > 0
        d = []
        for dual in (True, False):
            W = svc_weights(X, Y, dual=dual, random_state=0)
            d.append(np.linalg.norm((W - tight)[solved]) / np.linalg.norm(tight[solved]))
        dec = ls_cases.with_bias(X) @ tight.T
        tab, ce = [], []
        for a in range(Y.shape[1]):
            rows = Y[:, a] != 0
            svm_targets = (Y[rows, a] > 0).astype(np.int64)
            svm_outputs = (dec[rows, a] > 0).astype(np.int64) if solved[a] else svm_targets
            p = [[np.mean([case == (row, col) for case in zip(svm_outputs, svm_targets)]) for col in (0, 1)] for row in (0, 1)]
            tab.append(p)
            ce.append(ref['conditional_entropy'](p))
        out[name + '_W_tight'] = tight
        out[name + '_d_ref_dual_primal'] = np.array(d)
        out[name + '_d_ref'] = np.float64(min(d))
        out[name + '_tables'] = np.array(tab, dtype=np.float64)
        out[name + '_cond_entropy'] = np.array(ce, dtype=np.float64)
        print(name, 'd_ref dual %.3e primal %.3e' % tuple(d))
    np.savez_compressed(os.path.join(HERE, 'ls_golden.npz'), **out)


if __name__ == '__main__':
    main()
