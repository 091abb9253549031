#!/usr/bin/env python3
"""Quality metrics of a snapshot without a training run around it (reference: run_metrics.py:20-27 and its parser).

The networks whose pickles are not available here (Inception features / softmax, the attribute classifiers) are injected:
`inject` maps a constructor keyword (feature_fn, classify_fn, classify_fns) to a callable; on the command line
`--inject KEY=dotted.name` names it."""
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


def run(network_pkl, metrics, dataset, data_dir, mirror_augment, num_gpus=1, run_dir=None, inject=None):
    print('Evaluating metrics "%s" for "%s"...' % (','.join(metrics), network_pkl))
    network_pkl = pretrained_networks.get_path_or_url(network_pkl)
    dataset_args = dnnlib.EasyDict(tfrecord_dir=dataset, shuffle_mb=0, max_label_size='full')
    metric_group = metric_base.MetricGroup([_with_injected(metric_defaults[metric], inject) for metric in metrics])
    if run_dir is not None:
        os.makedirs(run_dir, exist_ok=True)
    metric_group.run(network_pkl, run_dir=run_dir, data_dir=data_dir, dataset_args=dataset_args, mirror_augment=mirror_augment, num_gpus=num_gpus)
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

    kwargs = vars(args)
    inject = {key: dnnlib.util.get_obj_by_name(name) for key, name in (kwargs.pop('inject') or [])}
    run_dir = next_run_dir(kwargs.pop('result_dir'), 'run-metrics')
    run(run_dir=run_dir, inject=inject, **kwargs)

#----------------------------------------------------------------------------

if __name__ == "__main__":
    main()
