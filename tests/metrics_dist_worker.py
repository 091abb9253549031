"""Worker process of the two-rank test of pr / prd / ppl (tests/test_gpu_metrics_ranks.py): the ranks share GPU 0 and talk
over gloo, as tests/class_dist_worker.py's do.  Also imported by the test itself for the pieces both sides must build alike
(generator, feature network, metric arguments).
usage: python tests/metrics_dist_worker.py <mode> <rank> <world> <port> <outdir> [<data_dir>]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from class_dist_worker import FMAP, RES, make_gs  # noqa: E402,F401

F = 24
NUM_IMAGES, MB = 40, 8
PPL_SAMPLES, PPL_MB = 10, 2
DATASET = dict(tfrecord_dir='reals', resolution=RES, max_label_size=0)
_PROJ = {}


def make_feature_fn(seen):
    """A deterministic device feature network: a fixed seeded projection of the uint8 image to F = 24 columns.  Appends the
    rows it returns to seen[seen['phase']]."""
    def feature_fn(images):
        dev = images.device
        if dev not in _PROJ:
            _PROJ[dev] = torch.randn(3 * RES * RES, F, device=dev, generator=torch.Generator(device=dev).manual_seed(24)) / 4000.0
        assert images.dtype == torch.uint8 and tuple(images.shape[1:]) == (3, RES, RES)
        f = images.float().reshape(images.shape[0], -1) @ _PROJ[dev]
        seen[seen['phase']].append(f.cpu().numpy())
        return f
    return feature_fn


def new_seen():
    return {name: dict(phase='real', real=[], fake=[]) for name in ('pr_tiny', 'prd_tiny')}


def metric_args(seen):
    """The three metrics as MetricGroup takes them; `seen`: new_seen(), filled by the feature networks."""
    return [dict(func_name='metrics.precision_recall.PR', name='pr_tiny', num_images=NUM_IMAGES, nhood_size=3, minibatch_per_gpu=MB,
                 row_batch_size=16, col_batch_size=16, feature_fn=make_feature_fn(seen['pr_tiny'])),
            dict(func_name='metrics.prd_score.PRD', name='prd_tiny', num_images=NUM_IMAGES, num_clusters=4, num_angles=11, num_runs=2,
                 minibatch_per_gpu=MB, feature_fn=make_feature_fn(seen['prd_tiny'])),
            dict(func_name='metrics.perceptual_path_length.PPL', name='ppl_tiny', num_samples=PPL_SAMPLES, epsilon=1e-2, space='w',
                 sampling='end', crop=False, minibatch_per_gpu=PPL_MB, Gs_overrides=dict(dtype='float32', mapping_dtype='float32'))]


def track_phase(metric, seen):
    """feature_fn files a row under the set (`which`) whose rows are being collected."""
    inner = metric._shard_feature_rows
    metric._shard_feature_rows = lambda Gs, Gs_kwargs, which, rank, world: (seen.__setitem__('phase', which), inner(Gs, Gs_kwargs, which, rank, world))[1]


def rows(seen_list):
    return np.concatenate(seen_list) if seen_list else np.zeros((0, F), dtype=np.float32)


def mode_metrics(rank, world, outdir, data_dir):
    """One MetricGroup.run of the three metrics under the world group."""
    from inclusivegan_amd.metrics import metric_base
    dev = torch.device('cuda', 0)
    Gs = make_gs(dev)
    seen = new_seen()
    group = metric_base.MetricGroup(metric_args(seen))
    for m in group.metrics[:2]:
        track_phase(m, seen[m.name])
    group.run(Gs, run_dir=outdir, data_dir=data_dir, dataset_args=dict(DATASET), mirror_augment=False,
              process_group=torch.distributed.group.WORLD)
    rec = dict(results={m.name: [(r.suffix, float(r.value)) for r in m._results] for m in group.metrics},
               fake={name: rows(seen[name]['fake']) for name in seen}, real={name: rows(seen[name]['real']) for name in seen})
    torch.save(rec, os.path.join(outdir, 'rank%d.pt' % rank))


def mode_loop(rank, world, outdir, data_dir):
    """Two iterations of the real training loop with a run directory (rank 0's) and a network snapshot at every tick; pr_tiny is
    evaluated by both ranks at each snapshot (modelled on tests/fid_dist_worker.py's snapshot case)."""
    from inclusivegan_amd.dnnlib import EasyDict
    from inclusivegan_amd.training import training_loop as TL
    B = 3
    state = dict(n=0)

    def on_iteration(info):
        state['n'] += 1
        return state['n'] >= 2

    seen = new_seen()
    metric = metric_args(seen)[0]
    res = TL.training_loop(
        G_args=EasyDict(func_name='training.networks_stylegan2.G_main', fmap_base=FMAP, architecture='skip'),
        D_args=EasyDict(func_name='training.networks_stylegan2.D_stylegan2_feature', fmap_base=FMAP, architecture='resnet'),
        G_opt_args=EasyDict(beta1=0.0, beta2=0.99, epsilon=1e-8), D_opt_args=EasyDict(beta1=0.0, beta2=0.99, epsilon=1e-8),
        G_loss_args=EasyDict(func_name='training.loss.G_logistic_ns_rec_interp_arb_pathreg', NN_rec_lpips_weight=2.5),
        D_loss_args=EasyDict(func_name='training.loss.D_logistic_r1', gamma=100),
        dataset_args=EasyDict(resolution=RES, num_channels=3, label_size=4, label_kind='attributes'),
        sched_args=EasyDict(minibatch_gpu_base=B, minibatch_size_base=B * world),
        metric_arg_list=[metric],
        run_dir=os.path.join(outdir, 'run') if rank == 0 else None,
        tf_config={'rnd.np_random_seed': 1000}, total_kimg=1, data_size=48, init_staleness=10, num_samples_factor=3,
        knn_perturb_factor=0.05, candidate_batch_size=16, hooks=dict(on_iteration=on_iteration))
    torch.save(dict(Gs=res['Gs'].flat_params.cpu(), feature_rows=int(sum(len(a) for a in seen['pr_tiny']['real'] + seen['pr_tiny']['fake']))),
               os.path.join(outdir, 'rank%d.pt' % rank))


def main():
    mode, rank, world, port, outdir = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    data_dir = sys.argv[6] if len(sys.argv) > 6 else None
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = port
    torch.cuda.set_device(0)
    torch.distributed.init_process_group('gloo', rank=rank, world_size=world)
    {'metrics': mode_metrics, 'loop': mode_loop}[mode](rank, world, outdir, data_dir)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
