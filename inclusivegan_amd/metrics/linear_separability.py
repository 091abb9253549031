"""Linear separability (reference: metrics/linear_separability.py:65-176; Karras et al., "A Style-Based Generator
Architecture for Generative Adversarial Networks").

    per attribute: keep the num_keep samples its classifier is most confident about, fit a linear SVM from the latent
    (z, or w = dlatents[:, -1]) to the classifier's decision, H(Y | X) of the (svm output, target) table in bits;
    score of a space = 2 ^ (sum of the conditional entropies over the attributes)                              (:149-176)

The reference fits sklearn.svm.LinearSVC() 80 times on one CPU core (40 attributes, two spaces, 100 000 x 512 each) and its
dual solver usually stops at max_iter without having converged.  Here the problem LinearSVC's defaults STATE is the
contract: squared hinge, L2, C = 1, the bias a regularised extra feature of value 1,

    f_a(w) = 1/2 |w|^2 + C * sum_{i kept for a} max(0, 1 - y_ai * w.(x_i, 1))^2,

strongly convex, so every attribute has one minimiser and that minimiser -- not a solver's iterate -- is what is computed.
All attributes of one space share the sample matrix, pruning is expressed as y = 0, and one batched Newton-CG solves them
together: gradient, Hessian-vector product and line search are one pass each over X for every attribute at once
(csrc/linear_svc.hip, exact-fp32 MFMA, fp64 fixed-order reductions), the [A, F + 1] vector algebra is fp64 on the device.

The 40 CelebA-HQ attribute classifiers of the reference (celebahq-classifier-00-male.pkl .. -39-wearing-necktie.pkl) are
not available; `LS` takes `classify_fns`: attribute index -> callable(float images [n, C, H, W] in G's range, box-mean
downsampled to 256 when larger) -> logits [n, 1].  With none injected it loads this project's own attribute classifier from
`classifier_pkl` (metrics/celeba_attribute_classifier.pkl, written by `python -m inclusivegan_amd.train_classifier --mode
attributes`): one network with one output per CelebA attribute, so a minibatch costs ONE forward and one pass of
hip_ops.binary_probs (csrc/sigmoid_xent.hip) instead of 40 forwards.  `ls` numbers obtained with that classifier are
comparable between models evaluated with the same pickle; they are not comparable to numbers obtained with the reference's
CelebA-HQ classifiers."""
import collections
import os

import numpy as np
import torch

from .. import hip_ops
from ..dnnlib.tflib import tfutil
from ..training.imle import CELEBA_ATTRIBUTES
from . import metric_base

DEFAULT_CLASSIFIER_PKL = 'metrics/celeba_attribute_classifier.pkl'      # relative to the working directory, as the Stacked-MNIST pickle

# The reference numbers its 40 classifiers in its own order (the file names in the comments of classifier_urls, :21-60): male,
# smiling, attractive, wavy hair, young, then CelebA's remaining 35 attributes alphabetically.  attrib_idx indexes THIS list;
# the column of a classifier trained on `dataset_tool.py create_celeba` labels is the name's place in imle.CELEBA_ATTRIBUTES.
LS_ATTRIBUTE_NAMES = tuple(
    'Male Smiling Attractive Wavy_Hair Young '
    '5_o_Clock_Shadow Arched_Eyebrows Bags_Under_Eyes Bald Bangs Big_Lips Big_Nose Black_Hair Blond_Hair Blurry Brown_Hair '
    'Bushy_Eyebrows Chubby Double_Chin Eyeglasses Goatee Gray_Hair Heavy_Makeup High_Cheekbones Mouth_Slightly_Open Mustache '
    'Narrow_Eyes No_Beard Oval_Face Pale_Skin Pointy_Nose Receding_Hairline Rosy_Cheeks Sideburns Straight_Hair Wearing_Earrings '
    'Wearing_Hat Wearing_Lipstick Wearing_Necklace Wearing_Necktie'.split())


def attribute_column(attrib_idx):
    """Column of imle.CELEBA_ATTRIBUTES that holds the attribute the reference numbers attrib_idx."""
    return CELEBA_ATTRIBUTES.index(LS_ATTRIBUTE_NAMES[attrib_idx])

# ---- information functions (:65-99), value for value: float32 normalisation, bits, the clamp at 0 ------------------------------


def prob_normalize(p):
    p = np.asarray(p).astype(np.float32)
    assert len(p.shape) == 2
    return p / np.sum(p)


def mutual_information(p):
    p = prob_normalize(p)
    px = np.sum(p, axis=1)
    py = np.sum(p, axis=0)
    result = 0.0
    for x in range(p.shape[0]):
        p_x = px[x]
        for y in range(p.shape[1]):
            p_xy = p[x][y]
            p_y = py[y]
            if p_xy > 0.0:
                result += p_xy * np.log2(p_xy / (p_x * p_y))     # bits
    return result


def entropy(p):
    p = prob_normalize(p)
    result = 0.0
    for x in range(p.shape[0]):
        for y in range(p.shape[1]):
            p_xy = p[x][y]
            if p_xy > 0.0:
                result -= p_xy * np.log2(p_xy)
    return result


def conditional_entropy(p):
    """H(Y | X), X on axis 0 and Y on axis 1; can slip just below 0 in floating point, hence the clamp (:94-99)."""
    p = prob_normalize(p)
    y = np.sum(p, axis=0, keepdims=True)
    return max(0.0, entropy(y) - mutual_information(p))


# ---- the batched solver -------------------------------------------------------------------------------------------------------

SvcFit = collections.namedtuple('SvcFit', 'W n_iter converged solved')
SvcFit.__doc__ = """W fp64 [A, F + 1] (bias last; zero rows for attributes that were not solved), Newton iterations per attribute,
converged (liblinear's primal stopping rule met), solved (False: the kept targets hold one class, nothing was fitted)."""

_GROUP = hip_ops.LINEAR_SVC_MAX_ATTRIBUTES
_STEPS = (0.0, 1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625)      # t = 0 first: the line search's own f(w)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('inclusivegan_amd linear separability needs a ROCm device; there is no CPU path')
    return torch.device('cuda', torch.cuda.current_device())


def _samples(X):
    dev = X.device if torch.is_tensor(X) and X.is_cuda else _device()
    X = torch.as_tensor(X).to(dev, torch.float32).contiguous()
    if X.dim() != 2:
        raise ValueError('X must be [n, F]')
    return X


def _dots(a, b):
    return torch.sum(a * b, dim=1)


class _Problem:
    """One group of at most 64 attributes on a shared X: buffers, and the three passes with the caller's halves added.

    The fp64 vectors of the solver are [A, P] with P = F + 1 rounded up to 16 and zeros in the padding: every row then starts
    at the same 128-byte alignment and has the same length, so a row-wise reduction runs the same program on every row and
    an attribute's result cannot depend on which row it occupies (with the odd pitch F + 1 = 513 it did)."""

    def __init__(self, X, Y, C):
        self.X, self.Y, self.C = X, Y, float(C)
        (self.n, self.F), self.A = X.shape, Y.shape[1]
        self.P = (self.F + 1 + 15) // 16 * 16
        dev = X.device
        self.ws = hip_ops.linear_svc_workspace(self.n, self.F, self.A, dev)
        self.dec = torch.empty((self.n, self.A), device=dev, dtype=torch.float32)
        self.z = torch.empty_like(self.dec)
        self.active = torch.empty((self.n, self.A), device=dev, dtype=torch.uint8)
        self.passes = dict(grad=0, hv=0, line=0)        # launches of each pass, for the record (tools/ls_bench.py)

    def _operand(self, V):
        return V[:, :self.F + 1].to(torch.float32).contiguous()

    def _padded(self, V):
        return torch.nn.functional.pad(V, (0, self.P - (self.F + 1)))

    def value_grad(self, W):
        """f and its gradient at W (fp64, fp32-representable); stores dec and the active mask."""
        self.passes['grad'] += 1
        loss, grad = hip_ops.linear_svc_grad_raw(self.X, self.Y, self._operand(W), self.dec, self.active, self.C, self.ws)
        return 0.5 * _dots(W, W) + self.C * loss, self._padded(grad) + W

    def hess_vec(self, S):
        """(I + 2C X_act^T X_act) S at the stored active mask; stores z = S.(x, 1)."""
        self.passes['hv'] += 1
        return self._padded(hip_ops.linear_svc_hv_raw(self.X, self.active, self._operand(S), self.z, self.C, self.ws)) + S

    def line_values(self, W, S, t):
        """f(W + t S) for step sizes t [T, A] from the stored dec and z."""
        self.passes['line'] += 1
        hinge = hip_ops.linear_svc_linesearch_raw(self.dec, self.z, self.Y, t, self.ws)
        moved = W.unsqueeze(0) + t.unsqueeze(2) * S.unsqueeze(0)
        return 0.5 * torch.sum(moved * moved, dim=2) + self.C * hinge


def _round32(v):
    return v.to(torch.float32).to(torch.float64)


def _conjugate_gradient(prob, g, run, gnorm, g0norm, max_cg):
    """H s = -g for the attributes in `run`, each with its own scalars; the others keep a zero step.  Forcing term
    sqrt(|g| / |g(0)|) (at most 0.1): superlinear outer convergence."""
    eta = torch.clamp(torch.sqrt(gnorm / torch.clamp(g0norm, min=1e-300)), min=1e-6, max=0.1)
    target = (eta * gnorm) ** 2
    s = torch.zeros_like(g)
    r = torch.where(run.unsqueeze(1), -g, torch.zeros_like(g))
    p = _round32(r)
    rr = _dots(r, r)
    for _ in range(max_cg):
        live = run & (rr > target)
        if not bool(live.any()):
            break
        p = torch.where(live.unsqueeze(1), p, torch.zeros_like(p))
        Hp = prob.hess_vec(p)
        alpha = torch.where(live, rr / torch.clamp(_dots(p, Hp), min=1e-300), torch.zeros_like(rr))
        s = s + alpha.unsqueeze(1) * p
        r = r - alpha.unsqueeze(1) * Hp
        rr_new = _dots(r, r)
        beta = torch.where(live, rr_new / torch.clamp(rr, min=1e-300), torch.zeros_like(rr))
        p = _round32(r + beta.unsqueeze(1) * p)
        rr = torch.where(live, rr_new, rr)
    return s


def _fit_group(X, Y, C, tol, max_iter, max_cg, stats=None):
    dev = X.device
    A, F = Y.shape[1], X.shape[1]
    pos = torch.sum(Y > 0, dim=0)
    neg = torch.sum(Y < 0, dim=0)
    solved = (pos > 0) & (neg > 0)
    prob = _Problem(X, (Y * solved.to(torch.int8).unsqueeze(0)).contiguous(), C)

    W = torch.zeros((A, prob.P), device=dev, dtype=torch.float64)
    f, g = prob.value_grad(W)
    gnorm = torch.sqrt(_dots(g, g))
    g0norm = gnorm.clone()
    # liblinear's primal rule with the reference's tol: |grad f(w)| <= tol * max(min(pos, neg), 1) / l * |grad f(0)|
    rule = tol * torch.clamp(torch.minimum(pos, neg), min=1).to(torch.float64) / torch.clamp(pos + neg, min=1).to(torch.float64) * g0norm
    run = solved & (g0norm > 0)
    best_W, best_g = W.clone(), gnorm.clone()
    n_iter = torch.zeros(A, device=dev, dtype=torch.int64)
    strikes = torch.zeros_like(n_iter)
    steps = torch.tensor(_STEPS, device=dev, dtype=torch.float64).unsqueeze(1).expand(len(_STEPS), A).contiguous()

    for _ in range(max_iter):
        if not bool(run.any()):
            break
        s = _round32(_conjugate_gradient(prob, g, run, gnorm, g0norm, max_cg))
        prob.hess_vec(s)                                   # z = s.(x, 1) for the line search
        gs = _dots(g, s)
        # Armijo on a grid: phi(t) = f(W + t s) is convex, so the candidate with the smallest value among those that pass is
        # taken; a direction from a small active set can need a step far below 1, hence up to four grids, 2^-7 apart.
        need = run & (gs < 0)
        found = torch.zeros_like(run)
        t = torch.zeros_like(gs)
        for depth in range(4):
            grid = steps * (2.0 ** (-7 * depth))            # row 0 stays t = 0: the line search's own f(W)
            phi = prob.line_values(W, s, grid)
            armijo = phi[1:] <= phi[0:1] + 1e-2 * grid[1:] * gs.unsqueeze(0)
            best = torch.argmin(torch.where(armijo, phi[1:], torch.full_like(phi[1:], float('inf'))), dim=0)
            pick = armijo.any(dim=0) & need & ~found
            t = torch.where(pick, grid[1:].gather(0, best.unsqueeze(0)).squeeze(0), t)
            found = found | pick
            if bool((found | ~need).all()):
                break
        W = _round32(W + t.unsqueeze(1) * s)
        f, g = prob.value_grad(W)
        gnorm = torch.sqrt(_dots(g, g))
        n_iter += run.to(torch.int64)
        # Iterate past the rule, down to where the fp32 products and the fp32-representable W stop improving the gradient: an
        # fp64 re-evaluation then still meets the rule.  An attribute is frozen (zero step from here on, its best iterate
        # kept) when its step failed, or when it is well inside the rule and three Newton steps have not halved its best.
        strikes = strikes + (run & (gnorm <= torch.minimum(0.25 * rule, 1e-6 * g0norm)) & (gnorm > 0.5 * best_g)).to(torch.int64)
        better = run & (gnorm < best_g)
        best_W = torch.where(better.unsqueeze(1), W, best_W)
        best_g = torch.where(better, gnorm, best_g)
        run = run & found & (strikes < 3) & (gnorm > 1e-13 * g0norm)
        W = torch.where(run.unsqueeze(1), W, best_W)
    converged = solved & (best_g <= 0.5 * rule)
    if stats is not None:
        for key, count in prob.passes.items():
            stats[key] = stats.get(key, 0) + count
    best_W = torch.where(solved.unsqueeze(1), best_W, torch.zeros_like(best_W))
    return best_W[:, :F + 1].contiguous(), n_iter, converged, solved


def linear_svc_fit(X, Y, C=1.0, tol=1e-4, max_iter=100, max_cg=250, stats=None):
    """Minimise f_a for every column a of Y on the shared samples X.

    X [n, F] fp32 (array or device tensor), Y [n, A] in {-1, 0, +1} (0 = the attribute has pruned the sample).  Newton-CG on the
    primal, Armijo backtracking, per-attribute scalars throughout; the stopping rule is liblinear's primal one with `tol`.
    An attribute whose kept targets hold one class is not solved (liblinear refuses it; the reference then takes the targets
    as predictions, :166-167).  `stats`: a dict that receives the number of gradient, Hessian-vector and line-search passes.
    -> SvcFit with host arrays."""
    X = _samples(X)
    Y = torch.as_tensor(Y).to(X.device, torch.int8)
    if Y.dim() != 2 or Y.shape[0] != X.shape[0]:
        raise ValueError('Y must be [n, A] with one row per sample')
    parts = [_fit_group(X, Y[:, a0:a0 + _GROUP].contiguous(), C, tol, int(max_iter), min(int(max_cg), 4 * (X.shape[1] + 1)), stats)
             for a0 in range(0, Y.shape[1], _GROUP)]
    W, n_iter, converged, solved = (torch.cat([p[i] for p in parts]).cpu().numpy() for i in range(4))
    return SvcFit(W, n_iter, converged, solved)


def linear_svc_decision(X, W):
    """dec fp32 device tensor [n, A] = W.(x, 1) on the kernels' own product."""
    X = _samples(X)
    W = torch.as_tensor(np.asarray(W, dtype=np.float64)).to(X.device, torch.float32)
    out = []
    for a0 in range(0, W.shape[0], _GROUP):
        Wg = W[a0:a0 + _GROUP].contiguous()
        A = Wg.shape[0]
        dec = torch.empty((X.shape[0], A), device=X.device, dtype=torch.float32)
        hip_ops.linear_svc_grad_raw(X, torch.zeros((X.shape[0], A), device=X.device, dtype=torch.int8), Wg, dec,
                                    torch.empty((X.shape[0], A), device=X.device, dtype=torch.uint8))
        out.append(dec)
    return torch.cat(out, dim=1).contiguous()


def linear_svc_predict(X, W):
    """Class index (dec > 0) of every sample under every attribute's weights -> int32 array [n, A]."""
    return hip_ops.linear_svc_predict_raw(linear_svc_decision(X, W)).cpu().numpy()


# ---- the metric ---------------------------------------------------------------------------------------------------------------

def prune_most_confident(predictions, num_keep):
    """Indices of the num_keep most confident samples, in the reference's order: a stable sort on -max probability, so lower
    indices win ties (:153-155).  predictions: device tensor [n, 2]."""
    conf = torch.max(predictions, dim=1).values
    return torch.sort(-conf, stable=True).indices[:num_keep]


def svm_targets_of(predictions):
    """argmax of the prediction pair, the first entry winning a tie as np.argmax does (:158)."""
    return (predictions[:, 1] > predictions[:, 0]).to(torch.int64)


def confusion_table(svm_outputs, svm_targets):
    """p[row][col] = share of samples with (svm output, target) == (row, col) (:170)."""
    svm_outputs, svm_targets = np.asarray(svm_outputs), np.asarray(svm_targets)
    return [[np.mean((svm_outputs == row) & (svm_targets == col)) for col in (0, 1)] for row in (0, 1)]


class LS(metric_base.MetricBase):
    def __init__(self, num_samples, num_keep, attrib_indices, minibatch_per_gpu, classify_fns=None, classifier_pkl=DEFAULT_CLASSIFIER_PKL, **kwargs):
        assert num_keep <= num_samples
        super().__init__(**kwargs)
        self.num_samples = num_samples
        self.num_keep = num_keep
        self.attrib_indices = attrib_indices
        self.minibatch_per_gpu = minibatch_per_gpu
        self.classify_fns = classify_fns        # injected functions always win; None: classifier_pkl is loaded when it exists
        self.classifier_pkl = classifier_pkl
        self.results = None             # what the sampling loop collected: latents, dlatents, attribute index -> [n, 2]
        self.fits = None                # space -> SvcFit of the last run

    def _collect(self, Gs, Gs_kwargs, minibatch_size):
        dev = Gs.device
        chunks = collections.defaultdict(list)
        for _begin in range(0, self.num_samples, minibatch_size):
            latents = tfutil.random_normal([minibatch_size] + Gs.input_shapes[0][1:], dev)
            labels = self._get_random_labels(minibatch_size, Gs)
            dlatents = Gs.components.mapping.get_output_for(latents, labels, **Gs_kwargs)
            images = Gs.get_output_for(latents, labels, **Gs_kwargs).to(torch.float32)
            if images.shape[2] > 256:       # the attribute classifiers were built for 256x256 (:128-131)
                factor = images.shape[2] // 256
                images = images.reshape(-1, images.shape[1], images.shape[2] // factor, factor, images.shape[3] // factor, factor).mean(dim=(3, 5))
            chunks['latents'].append(latents.to(torch.float32))
            chunks['dlatents'].append(dlatents[:, -1].to(torch.float32))
            if hasattr(self.classify_fns, 'classify_all'):      # one network, one output per attribute: one forward, one kernel
                logits = torch.as_tensor(self.classify_fns.classify_all(images)).to(dev, torch.float32).contiguous()
                probs = hip_ops.binary_probs(logits)            # [A, n, 2], attribute-major
                for attrib_idx in self.attrib_indices:
                    chunks[attrib_idx].append(probs[attribute_column(attrib_idx)])
                continue
            for attrib_idx in self.attrib_indices:
                logits = torch.as_tensor(self.classify_fns[attrib_idx](images)).to(dev, torch.float32).reshape(-1, 1)
                chunks[attrib_idx].append(torch.softmax(torch.cat([logits, -logits], dim=1), dim=1))
        return {key: torch.cat(value, dim=0)[:self.num_samples].contiguous() for key, value in chunks.items()}

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        attribs = list(self.attrib_indices)
        if self.classify_fns is None and self.classifier_pkl is not None and os.path.isfile(self.classifier_pkl):
            from ..train_classifier import load_attribute_classifier
            self.classify_fns = load_attribute_classifier(self.classifier_pkl, device=Gs.device)
            missing = [a for a in attribs if a not in self.classify_fns]
            if missing:
                raise RuntimeError('LS: the classifier of %s has %d outputs and none for attribute indices %s'
                                   % (self.classifier_pkl, self.classify_fns.num_attributes, missing))
        if self.classify_fns is None or any(a not in self.classify_fns for a in attribs):
            raise RuntimeError('LS needs classify_fns: the reference\'s celebahq-classifier-00-male.pkl .. '
                               'celebahq-classifier-39-wearing-necktie.pkl are not available in this tree')
        self.results = self._collect(Gs, Gs_kwargs, num_gpus * self.minibatch_per_gpu)
        dev = Gs.device

        # Prune the least confident samples of every attribute (y = 0) and take the classifier's decision as the target.
        Y = torch.zeros((self.num_samples, len(attribs)), device=dev, dtype=torch.int8)
        targets = torch.zeros((self.num_samples, len(attribs)), device=dev, dtype=torch.int64)
        for j, attrib_idx in enumerate(attribs):
            kept = prune_most_confident(self.results[attrib_idx], self.num_keep)
            targets[:, j] = svm_targets_of(self.results[attrib_idx])
            Y[kept, j] = (2 * targets[kept, j] - 1).to(torch.int8)
        kept_mask = (Y != 0).cpu().numpy()
        targets = targets.cpu().numpy()

        # One batched solve per space; the conditional entropy of every attribute's (svm output, target) table.
        conditional_entropies = collections.defaultdict(list)
        self.fits = {}
        for space in ['latents', 'dlatents']:
            fit = linear_svc_fit(self.results[space], Y)
            outputs = linear_svc_predict(self.results[space], fit.W)
            self.fits[space] = fit
            for j in range(len(attribs)):
                rows = kept_mask[:, j]
                svm_targets = targets[rows, j]
                svm_outputs = outputs[rows, j] if fit.solved[j] else svm_targets      # one class: assume perfect prediction
                conditional_entropies[space].append(conditional_entropy(confusion_table(svm_outputs, svm_targets)))

        scores = {key: 2 ** np.sum(values) for key, values in conditional_entropies.items()}
        self._report_result(scores['latents'], suffix='_z')
        self._report_result(scores['dlatents'], suffix='_w')
