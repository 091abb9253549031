#!/usr/bin/env python3
"""Quality metrics of a snapshot without a training run around it (reference: run_metrics.py:20-27 and its parser).

The networks whose pickles are not available here (Inception features / softmax, the attribute classifiers) are injected:
`inject` maps a constructor keyword (feature_fn, classify_fn, classify_fns) to a callable; on the command line
`--inject KEY=dotted.name` names it.  Without one, mode_counts* / KL* and ls load the classifiers train_classifier.py wrote under
metrics/ of the working directory (this project's own networks)."""
import argparse
import inspect
import os
import sys

from . import dnnlib
from . import pretrained_networks
from .dnnlib.util import next_run_dir
from .metrics import metric_base
from .metrics.metric_defaults import metric_defaults
from .run_training import _str_to_bool

#----------------------------------------------------------------------------

def _with_injected(metric_args, inject):
    """metric_args plus those entries of `inject` that the metric's constructor names as a keyword."""
    args = dnnlib.EasyDict(metric_args)
    if inject:
        cls = dnnlib.util.get_obj_by_name(metric_base._retarget(args)['func_name'])
        takes = inspect.signature(cls.__init__).parameters
        for key, value in inject.items():
            if key in takes and takes[key].kind in (inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY):
                args[key] = value
    return args


def run(network_pkl, metrics, dataset, data_dir, mirror_augment, num_gpus=1, run_dir=None, inject=None, process_group=None):
    """`process_group` None: this process evaluates everything (`num_gpus` scales the minibatch on its one device).  A group: every
    rank makes this call; metrics that spread over ranks (every one but ls) do, the others run on rank 0; pass `run_dir` on rank 0 only."""
    if process_group is None or run_dir is not None:
        print('Evaluating metrics "%s" for "%s"...' % (','.join(metrics), network_pkl))
    network_pkl = pretrained_networks.get_path_or_url(network_pkl)
    dataset_args = dnnlib.EasyDict(tfrecord_dir=dataset, shuffle_mb=0, max_label_size='full')
    metric_group = metric_base.MetricGroup([_with_injected(metric_defaults[metric], inject) for metric in metrics])
    if run_dir is not None:
        os.makedirs(run_dir, exist_ok=True)
    metric_group.run(network_pkl, run_dir=run_dir, data_dir=data_dir, dataset_args=dataset_args, mirror_augment=mirror_augment, num_gpus=num_gpus,
                     process_group=process_group)
    return metric_group

#----------------------------------------------------------------------------

def _parse_inject(s):
    key, sep, name = s.partition('=')
    if not sep or not key or not name:
        raise argparse.ArgumentTypeError('expected KEY=dotted.name')
    return key, name

#----------------------------------------------------------------------------

def build_parser():
    parser = argparse.ArgumentParser(
        description='Run StyleGAN2 metrics on MI355X.',
        formatter_class=argparse.RawDescriptionHelpFormatter
    )
    parser.add_argument('--metrics', help='Metrics to compute (default: %(default)s)', default='fid50k', type=lambda x: x.split(','))
    parser.add_argument('--data-dir', help='Dataset root directory', required=True)
    parser.add_argument('--dataset', help='Training dataset', required=True)
    parser.add_argument('--network', help='Network pickle filename', dest='network_pkl', required=True)
    parser.add_argument('--result-dir', help='Root directory for run results (default: %(default)s)', default='results', metavar='DIR')

    parser.add_argument('--mirror-augment', help='Mirror augment (default: %(default)s)', default=False, type=_str_to_bool, metavar='BOOL')
    parser.add_argument('--num-gpus', help='Number of GPUs to use', type=int, default=1, metavar='N')
    parser.add_argument('--inject', help='Network for a metric keyword (feature_fn, classify_fn, classify_fns) as KEY=dotted.name; repeatable',
                        action='append', default=None, type=_parse_inject, metavar='KEY=NAME')
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)

    if not os.path.exists(args.data_dir):
        print('Error: dataset root directory does not exist.')
        sys.exit(1)

    # one process per GPU, as run_training.main has it: the launcher sets RANK / WORLD_SIZE / LOCAL_RANK
    rank, world, local_rank = (int(os.environ.get(k, d)) for k, d in (('RANK', '0'), ('WORLD_SIZE', '1'), ('LOCAL_RANK', '0')))
    if args.num_gpus != world:
        print('Error: --num-gpus %d needs %d processes, one per GPU, and this job has %d.  Launch it as\n'
              '    python -m torch.distributed.run --nproc-per-node %d -m inclusivegan_amd.run_metrics --num-gpus %d ...'
              % (args.num_gpus, args.num_gpus, world, args.num_gpus, args.num_gpus))
        sys.exit(1)
    import torch
    torch.cuda.set_device(local_rank)
    process_group = None
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        import datetime
        # generous timeout: the metrics that do not spread over ranks run on rank 0 while the others wait at the closing barrier
        torch.distributed.init_process_group('nccl', timeout=datetime.timedelta(hours=4))
        process_group = torch.distributed.group.WORLD

    kwargs = vars(args)
    inject = {key: dnnlib.util.get_obj_by_name(name) for key, name in (kwargs.pop('inject') or [])}
    result_dir = kwargs.pop('result_dir')
    run_dir = next_run_dir(result_dir, 'run-metrics') if rank == 0 else None      # rank 0 alone creates it and reports into it
    run(run_dir=run_dir, inject=inject, process_group=process_group, **kwargs)
    if world > 1:
        torch.distributed.destroy_process_group()

#----------------------------------------------------------------------------

if __name__ == "__main__":
    main()
