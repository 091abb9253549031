"""Worker process of the multi-rank FID tests (tests/test_gpu_fid_merge.py): the ranks share GPU 0 and talk over gloo, as
tests/dist_worker.py's do.  Also imported by the test itself for the pieces both sides must build alike (generator, feature
network, metric object).
usage: python tests/fid_dist_worker.py <mode> <rank> <world> <port> <outdir> [<data_dir>]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

RES, FMAP, F = 32, 256, 192
NUM_IMAGES, MB = 100, 16
SYNTHETIC = dict(resolution=RES, num_channels=3, label_size=0, data_size=128)
_PROJ = {}

# what the feature network saw, in call order: the test process and the workers read it after a run
SEEN = dict(phase='real', real=[], fake=[], nan_in_fake=False)


def reset_seen(nan_in_fake=False):
    SEEN.update(phase='real', real=[], fake=[], nan_in_fake=nan_in_fake)


def make_gs(dev, label_size=0):
    from inclusivegan_amd.dnnlib import tflib
    return tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', num_channels=3,
                         resolution=RES, label_size=label_size, fmap_base=FMAP, device=dev, seed=5)


def feature_fn(images):
    """A deterministic device feature network with an importable name (the reals cache asks for one): a fixed seeded projection
    of the image to F = 192 columns.  Records the rows it returns under the current phase."""
    dev = images.device
    if dev not in _PROJ:
        _PROJ[dev] = torch.randn(3 * RES * RES, F, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) / 55.0
    assert images.dtype == torch.uint8 and tuple(images.shape[1:]) == (3, RES, RES)
    f = images.float().reshape(images.shape[0], -1) @ _PROJ[dev]
    if SEEN['nan_in_fake'] and SEEN['phase'] == 'fake' and not SEEN['fake']:
        f = f.clone()
        f[3, 5] = float('nan')
    SEEN[SEEN['phase']].append(f.cpu().numpy())
    return f


def make_fid(name='fid_tiny'):
    """The small FID entry; the phase of every feature_fn call is tracked at _shard_moments (group path) and _generate (single process)."""
    from inclusivegan_amd.metrics import frechet_inception_distance as FM
    fid = FM.FID(num_images=NUM_IMAGES, minibatch_per_gpu=MB, feature_fn=feature_fn, name=name)
    shard, generate = fid._shard_moments, fid._generate
    fid._shard_moments = lambda Gs, Gs_kwargs, which, rank, world: (SEEN.__setitem__('phase', which), shard(Gs, Gs_kwargs, which, rank, world))[1]
    fid._generate = lambda *a, **k: (SEEN.__setitem__('phase', 'fake'), generate(*a, **k))[1]
    fid.stats = {}
    merged = fid._merged_statistics

    def recorded(moments, device, what):
        fid.stats[what + '_rows'] = 0 if moments is None else int(moments.count)
        fid.stats[what] = merged(moments, device, what)
        return fid.stats[what]

    fid._merged_statistics = recorded
    return fid


def rows(kind, n):
    return np.concatenate(SEEN[kind])[:n] if SEEN[kind] else np.zeros((0, F), dtype=np.float32)


def mode_fid(rank, world, outdir, data_dir, nan_rank=None):
    """One FID evaluation under the world group; `data_dir`: a TFRecord set named 'reals' (cache enabled), else synthetic."""
    from inclusivegan_amd.training import misc
    dev = torch.device('cuda', 0)
    Gs = make_gs(dev)
    fid = make_fid()
    reset_seen(nan_in_fake=(rank == nan_rank))
    saves = []
    save_pkl = misc.save_pkl
    misc.save_pkl = lambda obj, path, *a, **k: (saves.append(path), save_pkl(obj, path, *a, **k))[1]
    dataset_args = dict(tfrecord_dir='reals', resolution=RES, max_label_size=0) if data_dir else SYNTHETIC
    rec = dict(error=None)
    try:
        fid.run(Gs, run_dir=outdir if rank == 0 else None, data_dir=data_dir, dataset_args=dataset_args, mirror_augment=False,
                process_group=torch.distributed.group.WORLD)
    except FloatingPointError as e:
        rec['error'] = str(e)
    n_real, n_fake = fid.stats.get('real_rows', 0), fid.stats.get('fake_rows', 0)
    rec.update(real=rows('real', n_real), fake=rows('fake', n_fake), real_rows=n_real, fake_rows=n_fake,
               results=[float(r.value) for r in fid._results], saves=saves,
               stats={k: v for k, v in fid.stats.items() if not k.endswith('_rows')})
    torch.save(rec, os.path.join(outdir, 'rank%d.pt' % rank))


def mode_fid_nan(rank, world, outdir, data_dir):
    mode_fid(rank, world, outdir, None, nan_rank=1)


def mode_loop(rank, world, outdir, data_dir, with_metric=True):
    """Two iterations of the real training loop with a run directory (rank 0's) and a network snapshot at every tick; the small
    FID entry evaluated by both ranks at each snapshot, or (`with_metric` False) no metric at all."""
    from inclusivegan_amd.dnnlib import EasyDict
    from inclusivegan_amd.training import training_loop as TL
    B = 3
    state = dict(n=0)

    def on_iteration(info):
        state['n'] += 1
        return state['n'] >= 2

    reset_seen()
    metric = dict(func_name='metrics.frechet_inception_distance.FID', name='fid_tiny', num_images=NUM_IMAGES, minibatch_per_gpu=MB, feature_fn=feature_fn)
    res = TL.training_loop(
        G_args=EasyDict(func_name='training.networks_stylegan2.G_main', fmap_base=FMAP, architecture='skip'),
        D_args=EasyDict(func_name='training.networks_stylegan2.D_stylegan2_feature', fmap_base=FMAP, architecture='resnet'),
        G_opt_args=EasyDict(beta1=0.0, beta2=0.99, epsilon=1e-8), D_opt_args=EasyDict(beta1=0.0, beta2=0.99, epsilon=1e-8),
        G_loss_args=EasyDict(func_name='training.loss.G_logistic_ns_rec_interp_arb_pathreg', NN_rec_lpips_weight=2.5),
        D_loss_args=EasyDict(func_name='training.loss.D_logistic_r1', gamma=100),
        dataset_args=EasyDict(resolution=RES, num_channels=3, label_size=4, label_kind='attributes'),
        sched_args=EasyDict(minibatch_gpu_base=B, minibatch_size_base=B * world),
        metric_arg_list=[metric] if with_metric else [],
        run_dir=os.path.join(outdir, 'run') if rank == 0 else None,
        tf_config={'rnd.np_random_seed': 1000}, total_kimg=1, data_size=24, init_staleness=10, num_samples_factor=3,
        knn_perturb_factor=0.05, candidate_batch_size=16, hooks=dict(on_iteration=on_iteration))
    torch.save(dict(G=res['G'].flat_params.cpu(), D=res['D'].flat_params.cpu(), Gs=res['Gs'].flat_params.cpu(),
                    feature_calls=len(SEEN['real']) + len(SEEN['fake'])), os.path.join(outdir, 'rank%d.pt' % rank))


def mode_loop_plain(rank, world, outdir, data_dir):
    mode_loop(rank, world, outdir, data_dir, with_metric=False)


def main():
    mode, rank, world, port, outdir = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    data_dir = sys.argv[6] if len(sys.argv) > 6 else None
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = port
    torch.cuda.set_device(0)
    torch.distributed.init_process_group('gloo', rank=rank, world_size=world)
    {'fid': mode_fid, 'fid_nan': mode_fid_nan, 'loop': mode_loop, 'loop_plain': mode_loop_plain}[mode](rank, world, outdir, data_dir)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
