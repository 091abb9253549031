#!/usr/bin/env python3
"""Image generation from a snapshot (reference: run_generator.py:19-37, generate-images): the same latent stream, the same
per-minibatch noise inputs, the same files.  The images leave the device as uint8 NHWC (tflib.convert_images_to_uint8 as
Gs.run's output transform) and are encoded by a fixed pool of writer threads while the next minibatch is generated."""
import argparse
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import PIL.Image

from . import dnnlib
from . import pretrained_networks
from .dnnlib import tflib
from .dnnlib.util import next_run_dir

NUM_PNG_WRITERS = 8     # fixed: a pool sized by the host's core count only slows itself down where the host is shared


def _save_png(image, path):
    if image.shape[-1] == 1:
        PIL.Image.fromarray(image[:, :, 0], 'L').save(path)
    else:
        PIL.Image.fromarray(image, 'RGB').save(path)


def generate_images(network_pkl, num_images, minibatch_size, truncation_psi=None, run_dir='.'):
    print('Loading networks from "%s"...' % network_pkl)
    Gs = pretrained_networks.load_networks(network_pkl)[-1]
    noise_vars = [var for name, var in Gs.components.synthesis.vars.items() if name.startswith('noise')]

    Gs_kwargs = dnnlib.EasyDict()
    Gs_kwargs.output_transform = dict(func=tflib.convert_images_to_uint8, nchw_to_nhwc=True)
    Gs_kwargs.randomize_noise = True
    if truncation_psi is not None:
        Gs_kwargs.truncation_psi = truncation_psi

    os.makedirs(run_dir, exist_ok=True)
    rnd = np.random.RandomState(0)
    with ThreadPoolExecutor(max_workers=NUM_PNG_WRITERS) as writers:
        jobs = []
        for image_idx in range(0, num_images, minibatch_size):
            z = rnd.randn(minibatch_size, *Gs.input_shape[1:])
            tflib.set_vars({var: rnd.randn(*[int(s) for s in var.shape]) for var in noise_vars})
            images = Gs.run(z, None, **Gs_kwargs)
            for i in range(minibatch_size):     # the last minibatch is written whole, like the reference's
                print('\rGenerating images (%d/%d) ...' % (image_idx+i, num_images), end='', flush=True)
                jobs.append(writers.submit(_save_png, images[i], os.path.join(run_dir, '%06d.png' % (image_idx+i))))
        for job in jobs:
            job.result()        # an encoding error surfaces here
    print()

#----------------------------------------------------------------------------

def _parse_num_range(s):
    """'a-c' -> range(a, c + 1); 'a,b,c' -> [a, b, c] (run_generator.py:41-49)."""
    m = re.match(r'^(\d+)-(\d+)$', s)
    if m is not None:
        lo, hi = (int(g) for g in m.groups())
        return range(lo, hi + 1)
    return [int(v) for v in s.split(',')]

#----------------------------------------------------------------------------

def build_parser():
    parser = argparse.ArgumentParser(
        description='''StyleGAN2 generator on MI355X.

Run 'python %(prog)s <subcommand> --help' for subcommand help.''',
        formatter_class=argparse.RawDescriptionHelpFormatter
    )
    subparsers = parser.add_subparsers(help='Sub-commands', dest='command')
    p = subparsers.add_parser('generate-images', help='Generate images')
    p.add_argument('--network', help='Network pickle filename', dest='network_pkl', required=True)
    p.add_argument('--result-dir', help='Root directory for run results (default: %(default)s)', default='generation', metavar='DIR')
    p.add_argument('--num-images', type=int, help='Number of images to generate (default: %(default)s)', default=30000)
    p.add_argument('--minibatch-size', type=int, help='Number of images per batch (default: %(default)s)', default=50)
    p.add_argument('--truncation-psi', type=float, help='Truncation psi (default: %(default)s)', default=None)
    return parser, {'generate-images': p}


def main(argv=None):
    parser, _ = build_parser()
    args = parser.parse_args(argv)
    kwargs = vars(args)
    subcmd = kwargs.pop('command')

    if subcmd is None:
        print('Error: missing subcommand.  Re-run with --help for usage.')
        sys.exit(1)

    run_dir = next_run_dir(kwargs.pop('result_dir'), subcmd)
    func_map = {'generate-images': generate_images}
    func_map[subcmd](run_dir=run_dir, **kwargs)

#----------------------------------------------------------------------------

if __name__ == "__main__":
    main()
