"""GPU: pr / prd / ppl evaluated by two ranks (tests/metrics_dist_worker.py: two fresh processes on GPU 0 over gloo) give,
on rank 0, the numbers of a one-process replay of both ranks' shares -- `==`, no tolerance: the searches are exact, the
gathers move bits, and the host statements run on identical arrays."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_world2(mode, outdir, data_dir=None, cwd=ROOT, timeout=600):
    """2 ranks of tests/metrics_dist_worker.py, each started fresh and waited for, none retried; -> the ranks' records."""
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, os.path.join(ROOT, 'tests', 'metrics_dist_worker.py'), mode]
    procs = [subprocess.Popen(cmd + [str(r), '2', str(port), str(outdir)] + ([str(data_dir)] if data_dir else []),
                              cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=timeout) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    return [torch.load(os.path.join(str(outdir), 'rank%d.pt' % r), weights_only=False) for r in range(2)], [so for so, _ in outs]


def test_two_ranks_evaluate_pr_prd_ppl(cuda_device, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import metrics_dist_worker as W
    from inclusivegan_amd.metrics import metric_base, prd_score
    from inclusivegan_amd.metrics import perceptual_path_length as PPLM
    from inclusivegan_amd.metrics import precision_recall as PRM
    from inclusivegan_amd.metrics.frechet_inception_distance import shard_slices
    from inclusivegan_amd.training import tfrecord
    rng = np.random.RandomState(3)
    os.makedirs(str(tmp_path / 'data' / 'reals'))
    with tfrecord.TFRecordExporter(str(tmp_path / 'data' / 'reals'), 64, print_progress=False) as tfr:
        for _ in range(64):
            tfr.add_image(rng.randint(0, 256, size=(3, 32, 32)).astype(np.uint8))
    work = tmp_path / 'work'
    work.mkdir()
    (r0, r1), _ = run_world2('metrics', tmp_path, data_dir=tmp_path / 'data', cwd=work)

    # rank 0 alone holds results and wrote one line per metric
    assert [s for s, _ in r0['results']['pr_tiny']] == ['_precision', '_recall']
    assert [s for s, _ in r0['results']['prd_tiny']] == ['_F8', '_F1_8']
    assert [s for s, _ in r0['results']['ppl_tiny']] == ['']
    assert all(v == [] for v in r1['results'].values())
    for name in ('pr_tiny', 'prd_tiny', 'ppl_tiny'):
        with open(str(tmp_path / ('metric-%s.txt' % name))) as f:
            lines = f.read().strip().splitlines()
        assert len(lines) == 1 and name in lines[0]

    # the shares of both ranks, rebuilt in this process
    dev = cuda_device
    Gs = W.make_gs(dev)
    Gs_kwargs = dict(is_validation=True)
    seen = W.new_seen()
    pr, prd, ppl = metric_base.MetricGroup(W.metric_args(seen)).metrics
    slices = [shard_slices(W.NUM_IMAGES, W.MB, r, 2) for r in range(2)]
    assert slices[1][2] == (40, 40)                     # rank 1 sits the third global minibatch out
    for m in (pr, prd):
        m._configure('live-network', str(tmp_path / 'data'), dict(W.DATASET), False)
        feature_fn = m.feature_fn
        placed = {}
        for which in ('real', 'fake'):
            placed[which] = torch.full([W.NUM_IMAGES, W.F], float('nan'), device=dev)
            for r, rec in enumerate((r0, r1)):
                if which == 'fake':                         # through _fold_shard_fakes with the same (rank, world)
                    got = []
                    m._fold_shard_fakes(Gs, Gs_kwargs, r, 2, lambda b, e, images: got.append((b, e, feature_fn(images))))
                else:
                    got = m._shard_feature_rows(Gs, Gs_kwargs, which, r, 2)
                assert [(b, e) for b, e, _ in got] == [s for s in slices[r] if s[1] > s[0]]
                mine = torch.cat([f for _, _, f in got]).cpu().numpy()
                assert mine.shape == (24 if r == 0 else 16, W.F)
                assert rec[which][m.name].tobytes() == mine.tobytes(), (m.name, which, r)     # what the rank's feature_fn saw
                for b, e, f in got:
                    placed[which][b:e] = f
            assert bool(torch.isfinite(placed[which]).all())
        if m is pr:
            state = PRM.knn_precision_recall_features(placed['real'], placed['fake'], nhood_sizes=[3], row_batch_size=16, col_batch_size=16)
            want = [float(state.knn_precision[0]), float(state.knn_recall[0])]
        else:
            precision, recall = prd_score.compute_prd_from_embedding(placed['fake'], placed['real'], num_clusters=4, num_angles=11, num_runs=2, seed=0)
            want = [float(v) for v in prd_score.prd_to_max_f_beta_pair(precision, recall, beta=8)]
        print(m.name, want, [v for _, v in r0['results'][m.name]])
        assert [v for _, v in r0['results'][m.name]] == want, m.name
        m.close()

    # PPL: rank 0 owns three of the five minibatches, rank 1 two; re-interleaved in order of g
    T = PPLM.num_minibatches(W.PPL_SAMPLES, W.PPL_MB)
    per_rank = [ppl.rank_distances(Gs, Gs_kwargs, r, 2).cpu().numpy() for r in range(2)]
    assert T == 5 and [len(d) for d in per_rank] == [3, 2]
    flat = np.concatenate([per_rank[g % 2][g // 2] for g in range(T)])
    want = float(np.mean(PPLM.reject_outliers(flat)))
    print('ppl_tiny', want, r0['results']['ppl_tiny'][0][1])
    assert np.isfinite(want) and r0['results']['ppl_tiny'][0][1] == want
    # the two ranks drew different pairs
    assert not np.array_equal(per_rank[0][0], per_rank[1][0])


def test_training_loop_evaluates_pr_on_both_ranks(cuda_device, tmp_path):
    """World 2, two iterations, a network snapshot at every tick with pr_tiny: rank 0 writes one result line per snapshot, both
    ranks computed features, and both leave together with the same Gs."""
    (r0, r1), _ = run_world2('loop', tmp_path, timeout=900)
    snapshots = [f for f in os.listdir(str(tmp_path / 'run')) if f.startswith('network-snapshot-')]
    with open(str(tmp_path / 'run' / 'metric-pr_tiny.txt')) as f:
        lines = f.read().strip().splitlines()
    assert len(snapshots) >= 1 and len(lines) == len(snapshots)
    assert all('pr_tiny_precision' in ln and 'pr_tiny_recall' in ln for ln in lines)
    assert r0['feature_rows'] > 0 and r1['feature_rows'] > 0
    assert torch.equal(r0['Gs'], r1['Gs'])
