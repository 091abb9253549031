"""Worker process of the multi-rank classifier-metric test (tests/test_gpu_class_stats.py): the ranks share GPU 0 and talk
over gloo, as tests/fid_dist_worker.py's do.  Also imported by the test itself for the pieces both sides must build alike
(generator, stand-in classifiers, metric arguments).
usage: python tests/class_dist_worker.py <mode> <rank> <world> <port> <outdir>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

RES, FMAP = 32, 256
K_LOGITS, K_PROBS = 101, 37
NUM_IMAGES, MB, SPLITS = 30, 8, 3
_PROJ = {}


def make_gs(dev, label_size=0):
    from inclusivegan_amd.dnnlib import tflib
    return tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', architecture='skip', num_channels=3,
                         resolution=RES, label_size=label_size, fmap_base=FMAP, device=dev, seed=5)


def _proj(dev, K):
    if (dev, K) not in _PROJ:
        _PROJ[(dev, K)] = torch.randn(3 * RES * RES, K, device=dev, generator=torch.Generator(device=dev).manual_seed(K)) / 8.0
    return _PROJ[(dev, K)]


def make_logits_fn(seen, to_host=False):
    """A deterministic stand-in for the Stacked-MNIST classifier: a fixed seeded projection of the float image to K_LOGITS
    logits.  Appends the rows it returns to `seen`."""
    def classify(images):
        assert images.dtype == torch.float32 and tuple(images.shape[1:]) == (3, RES, RES)
        logits = images.reshape(images.shape[0], -1) @ _proj(images.device, K_LOGITS)
        seen.append(logits.cpu().numpy())
        return logits.cpu() if to_host else logits
    return classify


def make_probs_fn(seen, to_host=False):
    """A stand-in for the Inception softmax: uint8 images -> K_PROBS probabilities, none of them zero."""
    def classify(images):
        assert images.dtype == torch.uint8 and tuple(images.shape[1:]) == (3, RES, RES)
        x = images.to(torch.float32).reshape(images.shape[0], -1) / 255.0 - 0.5
        probs = torch.softmax(x @ _proj(images.device, K_PROBS), dim=1)
        seen.append(probs.cpu().numpy())
        return probs.cpu() if to_host else probs
    return classify


def metric_args(seen, num_images=NUM_IMAGES, mb=MB, to_host=False):
    """The three metrics as MetricGroup takes them; `seen`: dict of lists, one per metric, filled by the classifiers."""
    return [dict(func_name='metrics.mode_counts.mode_counts', name='modes_tiny', num_images=num_images, minibatch_per_gpu=mb,
                 classify_fn=make_logits_fn(seen['modes_tiny'], to_host)),
            dict(func_name='metrics.KL.KL', name='kl_tiny', num_images=num_images, minibatch_per_gpu=mb,
                 classify_fn=make_logits_fn(seen['kl_tiny'], to_host)),
            dict(func_name='metrics.inception_score.IS', name='is_tiny', num_images=num_images, num_splits=SPLITS, minibatch_per_gpu=mb,
                 classify_fn=make_probs_fn(seen['is_tiny'], to_host))]


def new_seen():
    return dict(modes_tiny=[], kl_tiny=[], is_tiny=[])


def rows(seen_list, K):
    return np.concatenate(seen_list) if seen_list else np.zeros((0, K), dtype=np.float32)


def mode_metrics(rank, world, outdir):
    """One MetricGroup.run of the three metrics under the world group."""
    from inclusivegan_amd.metrics import metric_base
    dev = torch.device('cuda', 0)
    Gs = make_gs(dev)
    seen = new_seen()
    group = metric_base.MetricGroup(metric_args(seen))
    group.run(Gs, run_dir=outdir, process_group=torch.distributed.group.WORLD)
    rec = dict(results={m.name: [(r.suffix, float(r.value)) for r in m._results] for m in group.metrics},
               rows={name: rows(seen[name], K_PROBS if name == 'is_tiny' else K_LOGITS) for name in seen})
    torch.save(rec, os.path.join(outdir, 'rank%d.pt' % rank))


def main():
    mode, rank, world, port, outdir = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = port
    torch.cuda.set_device(0)
    torch.distributed.init_process_group('gloo', rank=rank, world_size=world)
    {'metrics': mode_metrics}[mode](rank, world, outdir)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
