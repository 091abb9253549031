"""GPU: the walk over reals and fakes of FID, IS, mode_counts, KL, PR and PRD, as literal transcripts -- how many rows the
injected network saw in every call, how many rows the generator and the label draw were asked for, which label rows a rank's
generator call received -- in one process (num_gpus 1 and 2) and for every rank of a world replayed in this process through
the per-rank entry points.  Where the ragged last minibatch is cut is part of the transcript (metric_base.MetricBase._walk).

The test goes through `run()`, `MetricBase._feature_matrix` and the per-rank entry points only.  It also PRINTS (and does not
assert: the bytes depend on the platform) SHA-1 digests of every recorded network output and of every final state or result;
run with -rP, the `digest` lines of two trees on one library are an A/B record (profiles/metric_walks.txt)."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 32
SYNTHETIC = dict(resolution=RES, num_channels=3, label_size=4, data_size=64)
KWARGS = dict(is_validation=True)
NAMES = ('fid', 'is', 'modes', 'kl', 'pr', 'prd')
WITH_REALS = ('fid', 'pr', 'prd')
_PROJ = {}


@pytest.fixture(autouse=True)
def _no_grad():
    """As MetricBase.run evaluates; the per-rank entry points are called outside run()."""
    was = torch.is_grad_enabled()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(was)


def make_gs(dev):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import fid_dist_worker
    return fid_dist_worker.make_gs(dev, label_size=4)        # conditional: the label dealing is part of what is seen


def digest(tag, *arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        h.update(np.ascontiguousarray(a).tobytes())
    print('digest %s %s' % (tag, h.hexdigest()))


class Watch:
    """One metric under observation: `net` is its injected network (a fixed seeded projection of the image to K columns, a
    softmax on top for 'probs'), `_generate` and `_get_random_labels` are wrapped.  Everything is filed in call order."""

    def __init__(self, kind, K, to_host=False):
        self.kind, self.K, self.to_host = kind, K, to_host
        self.phase = 'real'
        self.seen = dict(real=[], fake=[])      # the network's outputs, one array per call
        self.generated = []                     # rows every _generate call was asked for
        self.labels_given = []                  # the `labels=` of every _generate call (None: drawn inside)
        self.labels_asked = []                  # rows every _get_random_labels call was asked for

    def net(self, images):
        dev = images.device
        if (dev, self.K) not in _PROJ:
            _PROJ[(dev, self.K)] = torch.randn(3 * RES * RES, self.K, device=dev, generator=torch.Generator(device=dev).manual_seed(self.K)) / 8.0
        assert images.dtype == (torch.float32 if self.kind == 'logits' else torch.uint8) and tuple(images.shape[1:]) == (3, RES, RES)
        x = images.reshape(images.shape[0], -1).to(torch.float32)
        if self.kind != 'logits':
            x = x / 255.0 - 0.5
        out = x @ _PROJ[(dev, self.K)]
        if self.kind == 'probs':
            out = torch.softmax(out, dim=1)
        self.seen[self.phase].append(out.cpu().numpy())
        return out.cpu().numpy() if self.to_host else out

    def attach(self, metric):
        generate, labels = metric._generate, metric._get_random_labels

        def watched_generate(Gs, minibatch_size, *args, **kwargs):
            self.phase = 'fake'
            self.generated.append(minibatch_size)
            given = kwargs.get('labels')
            self.labels_given.append(None if given is None else given.cpu().numpy())
            return generate(Gs, minibatch_size, *args, **kwargs)

        def watched_labels(minibatch_size, Gs):
            self.labels_asked.append(minibatch_size)
            return labels(minibatch_size, Gs)

        metric._generate, metric._get_random_labels = watched_generate, watched_labels
        self.metric = metric
        return metric

    def rows(self, which):
        return [a.shape[0] for a in self.seen[which]]

    def print_digests(self, tag):
        for which in ('real', 'fake'):
            for i, a in enumerate(self.seen[which]):
                digest('%s %s call %d rows %d' % (tag, which, i, a.shape[0]), a)


def make_metric(name, num_images, mb, to_host=False):
    from inclusivegan_amd.metrics import KL, frechet_inception_distance, inception_score, mode_counts, prd_score, precision_recall
    if name == 'fid':
        w = Watch('features', 24, to_host)
        return w, w.attach(frechet_inception_distance.FID(num_images=num_images, minibatch_per_gpu=mb, feature_fn=w.net, name='fid_walk'))
    if name == 'is':
        w = Watch('probs', 37, to_host)
        return w, w.attach(inception_score.IS(num_images=num_images, num_splits=3, minibatch_per_gpu=mb, classify_fn=w.net, name='is_walk'))
    if name in ('modes', 'kl'):
        w = Watch('logits', 101, to_host)
        cls = mode_counts.mode_counts if name == 'modes' else KL.KL
        return w, w.attach(cls(num_images=num_images, minibatch_per_gpu=mb, classify_fn=w.net, name=name + '_walk'))
    if name == 'pr':
        w = Watch('features', 24, to_host)
        return w, w.attach(precision_recall.PR(num_images=num_images, nhood_size=3, minibatch_per_gpu=mb, row_batch_size=16, col_batch_size=16,
                                               feature_fn=w.net, name='pr_walk'))
    w = Watch('features', 24, to_host)
    return w, w.attach(prd_score.PRD(num_images=num_images, num_clusters=20, num_angles=1001, num_runs=10, minibatch_per_gpu=mb,
                                     feature_fn=w.net, name='prd_walk'))


# ---- one process --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('num_gpus,reals,fakes', [(1, [8, 8, 4], [8, 8, 8]), (2, [16, 4], [16, 16])])
def test_one_process_transcripts(cuda_device, num_gpus, reals, fakes):
    """20 images, minibatch_per_gpu 8: the reals are cut to the images that are left BEFORE the network, of the fakes the
    network sees whole minibatches and its RESULT is cut (the reference's statement)."""
    Gs = make_gs(cuda_device)
    for name in NAMES:
        w, m = make_metric(name, 20, 8)
        tag = 'one_process num_gpus=%d %s' % (num_gpus, name)
        if name == 'prd':       # 20 rows cannot be clustered into the metric's 20 bins twice over: the feature collection alone
            m._configure('live-network', None, dict(SYNTHETIC), False)
            real = m._feature_matrix(Gs, KWARGS, 'real', num_gpus)
            fake = m._feature_matrix(Gs, KWARGS, 'fake', num_gpus)
            assert real.is_cuda and real.dtype == torch.float32 and tuple(real.shape) == tuple(fake.shape) == (20, 24)
            digest(tag + ' matrices', real, fake)
        else:
            m.run(Gs, dataset_args=dict(SYNTHETIC), mirror_augment=False, num_gpus=num_gpus, log_results=False)
            assert len(m._results) >= 1
            digest(tag + ' results', np.asarray([r.value for r in m._results], dtype=np.float64))
        assert w.rows('real') == (reals if name in WITH_REALS else []), name
        assert w.rows('fake') == fakes, name
        assert w.generated == fakes and w.labels_asked == fakes, name
        assert all(given is None for given in w.labels_given), name       # one process: _generate draws its own labels
        w.print_digests(tag)
        m.close()


# ---- every rank of a world, replayed in this process ---------------------------------------------------------------------------
def shard_state(name, m, w, Gs, which, rank, world):
    """What the per-rank entry point of the metric returns for the 'real' or 'fake' images of rank `rank` of `world`."""
    from inclusivegan_amd.metrics import mode_counts
    w.phase = which
    if name == 'fid':
        return m._shard_moments(Gs, KWARGS, which, rank, world)
    if name in ('pr', 'prd'):
        return m._shard_feature_rows(Gs, KWARGS, which, rank, world)
    assert which == 'fake'
    if name == 'is':
        return m._shard_stats(Gs, KWARGS, rank, world)
    return mode_counts.shard_histogram(m, Gs, KWARGS, rank, world)


def drawn_labels(count, rounds):
    """`rounds` consecutive draws of `count` label rows from the label stream's seed through the data set."""
    from inclusivegan_amd.training import dataset
    ds = dataset.load_dataset(data_dir=None, **SYNTHETIC)
    rng = np.random.RandomState(0x1ab)
    return [np.asarray(ds.get_random_labels_np(count, rng=rng), dtype=np.float32) for _ in range(rounds)]


def print_merged(tag, name, states, num_images, dev):
    """Digests of the ranks' states folded together (the moments / sums / counts), or of their rows in place."""
    from inclusivegan_amd import hip_ops
    states = [s for s in states if s is not None]
    if name == 'fid':
        total = hip_ops.FeatureMoments(states[0].F, dev)
        for s in states:
            total.merge(s)
        assert total.count == num_images
        digest(tag + ' mu sigma', *total.finalize())
    elif name == 'is':
        total = hip_ops.SplitProbStats(states[0].K, num_images, 3, dev)
        for s in states:
            total.merge(s)
        assert sum(total.n) == num_images
        digest(tag + ' psum plogp scores', total.psum, total.plogp, np.asarray(total.scores(), dtype=np.float64))
    elif name in ('modes', 'kl'):
        total = hip_ops.ClassHistogram(states[0].K, dev)
        for s in states:
            total.merge(s)
        assert total.count == num_images
        digest(tag + ' counts', total.to_host())
    else:
        placed = torch.full([num_images, 24], float('nan'), device=dev)
        for rows in states:
            for b, e, f in rows:
                assert f.dtype == torch.float32 and tuple(f.shape) == (e - b, 24)
                placed[b:e] = f
        assert bool(torch.isfinite(placed).all())
        digest(tag + ' matrix', placed)


def replay(dev, world, num_images, mb, want):
    """Every metric, every rank; `want(name, rank)` -> (rows of the reals' network calls, of the fakes', generator calls)."""
    Gs = make_gs(dev)
    rounds = -(-num_images // (world * mb))
    draws = drawn_labels(world * mb, rounds)
    for name in NAMES:
        states = dict(real=[], fake=[])
        for rank in range(world):
            w, m = make_metric(name, num_images, mb)
            m._configure('live-network', None, dict(SYNTHETIC), False)
            real = shard_state(name, m, w, Gs, 'real', rank, world) if name in WITH_REALS else None
            fake = shard_state(name, m, w, Gs, 'fake', rank, world)
            tag = 'world=%d rank=%d %s' % (world, rank, name)
            reals, fakes, calls = want(name, rank)
            assert w.rows('real') == (reals if name in WITH_REALS else []), tag
            assert w.rows('fake') == fakes, tag
            assert w.generated == [mb] * calls, tag
            # labels: drawn for the whole global minibatch in every round, also by a rank that sits it out; the generator gets
            # the rank's rows of that draw
            assert w.labels_asked == [world * mb] * rounds, tag
            assert len(w.labels_given) == calls
            for g, given in enumerate(w.labels_given):
                assert given.tobytes() == draws[g][rank * mb:(rank + 1) * mb].tobytes(), tag
            if not fakes:       # a rank without a row
                assert fake is None or fake == [], tag
                assert real is None or real == [], tag
            w.print_digests(tag)
            states['real'].append(real if real != [] else None)
            states['fake'].append(fake if fake != [] else None)
            m.close()
        if name in WITH_REALS:
            print_merged('world=%d %s real' % (world, name), name, states['real'], num_images, dev)
        print_merged('world=%d %s fake' % (world, name), name, states['fake'], num_images, dev)


def test_world_2_transcripts(cuda_device):
    """30 images, mb 8: rank 1's last slice has 6 rows.  The reals are cut before the network everywhere.  Of the fakes FID
    gives the network the whole minibatch and cuts the result, the other five cut the images first: today's table, pinned."""
    def want(name, rank):
        if rank == 0:
            return [8, 8], [8, 8], 2
        return [8, 6], ([8, 8] if name == 'fid' else [8, 6]), 2
    replay(cuda_device, 2, 30, 8, want)


def test_world_4_transcripts_with_a_rank_that_owns_nothing(cuda_device):
    """7 images, mb 3: the ranks own 3, 3, 1, 0 rows.  Rank 3 returns nothing, never calls the generator and still draws the
    labels of the one global minibatch, 12 rows."""
    from inclusivegan_amd.metrics.frechet_inception_distance import shard_slices
    assert [sum(e - b for b, e in shard_slices(7, 3, r, 4)) for r in range(4)] == [3, 3, 1, 0]

    def want(name, rank):
        if rank == 3:
            return [], [], 0
        if rank == 2:
            return [1], ([3] if name == 'fid' else [1]), 1
        return [3], [3], 1
    replay(cuda_device, 4, 7, 3, want)


def test_a_refusal_inside_a_sharded_walk_ends_the_private_random_source(cuda_device):
    """A network that returns NumPy is refused under a group, from inside the walk over the fakes; the process's random source
    is the one it was, although pytest.raises keeps the traceback and its frames alive."""
    from inclusivegan_amd.dnnlib.tflib import tfutil
    Gs = make_gs(cuda_device)
    before = tfutil._random
    kept = []
    for name in NAMES:
        w, m = make_metric(name, 30, 8, to_host=True)
        m._configure('live-network', None, dict(SYNTHETIC), False)
        with pytest.raises(RuntimeError, match='must return (float32 )?device tensors') as caught:
            shard_state(name, m, w, Gs, 'fake', 1, 2)
        kept.append(caught)
        assert w.generated == [8] and w.rows('fake') == [8]      # refused at the first minibatch
        assert tfutil._random is before, name
        m.close()
    assert tfutil._random is before
