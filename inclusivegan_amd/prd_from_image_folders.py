#!/usr/bin/env python3
"""PRD of image folders (reference: precision-recall-distributions/prd_from_image_folders.py): F_1/8 (precision) and F_8
(recall) of every --eval_dirs folder against --reference_dir, printed as the reference's table.

The reference embeds the images with a frozen Inception graph (inception.pb) that is not available here; the embedding
network is injected instead, `--inject feature_fn=dotted.name`: a callable taking uint8 images [n, C, H, W] on the device and
returning [n, F] features, as for `run_metrics --metrics fid30k`.  Images are read with PIL in sorted file order (the
reference: OpenCV in directory order) and embeddings are cached as <cache_dir>/<md5 of the directory path>.npy like the
reference's.  `--plot_path` and `--inception_path` are accepted and ignored.  Nothing here opens a connection."""
import argparse
import hashlib
import os

import numpy as np

from .metrics import prd_score as prd
from .run_metrics import _parse_inject

IMAGE_TYPES = ('png', 'jpg', 'bmp', 'gif')


def build_parser():
    """The reference's flags (same names, types and defaults) plus --inject, --seed and --batch_size."""
    parser = argparse.ArgumentParser(description='PRD (F_1/8 precision, F_8 recall) of image folders on MI355X.',
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument('--reference_dir', type=str, required=True, help='folder of real images')
    parser.add_argument('--eval_dirs', type=str, nargs='+', required=True, help='one or more folders of generated images')
    parser.add_argument('--eval_labels', type=str, nargs='+', required=True, help='one label per --eval_dirs folder')
    parser.add_argument('--num_clusters', type=int, default=20, help='bins of the k-means partition')
    parser.add_argument('--num_angles', type=int, default=1001, help='slopes of the PRD curve, in [3, 1e6]')
    parser.add_argument('--num_runs', type=int, default=10, help='independent clusterings whose curves are averaged')
    parser.add_argument('--plot_path', type=str, default=None, help='accepted and ignored: no plot is made')
    parser.add_argument('--cache_dir', type=str, default='/tmp/prd_cache/', help='where embeddings are cached per folder')
    parser.add_argument('--inception_path', type=str, default='precision-recall-distributions/inception.pb',
                        help='accepted and ignored: the embedding network is --inject feature_fn=...')
    parser.add_argument('--silent', dest='verbose', action='store_false', help='no progress lines')
    parser.add_argument('--inject', help='the embedding network as feature_fn=dotted.name', action='append', default=None,
                        type=_parse_inject, metavar='KEY=NAME')
    parser.add_argument('--seed', type=int, default=0, help='seed of the clustering draws')
    parser.add_argument('--batch_size', type=int, default=64, help='images per call of the embedding network')
    return parser


def load_images_from_dir(directory, types=IMAGE_TYPES):
    """uint8 [n, H, W, 3] RGB images of a folder, in sorted file order."""
    import PIL.Image
    names = sorted(fn for fn in os.listdir(directory) if os.path.splitext(fn)[-1][1:] in types)
    if not names:
        raise ValueError('no images (%s) in %s' % (', '.join(types), directory))
    imgs = [np.asarray(PIL.Image.open(os.path.join(directory, fn)).convert('RGB')) for fn in names]
    return np.array(imgs)


def generate_embedding(imgs, feature_fn, batch_size=64):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('inclusivegan_amd PRD needs a ROCm device; there is no CPU path')
    dev = torch.device('cuda', torch.cuda.current_device())
    out = []
    for begin in range(0, len(imgs), batch_size):
        batch = torch.from_numpy(np.ascontiguousarray(imgs[begin:begin + batch_size].transpose(0, 3, 1, 2))).to(dev)
        f = feature_fn(batch)
        out.append(f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f))
    return np.concatenate(out).astype(np.float32)


def load_or_generate_embedding(directory, cache_dir, feature_fn, batch_size=64):
    hash = hashlib.md5(directory.encode('utf-8')).hexdigest()
    path = os.path.join(cache_dir, hash + '.npy')
    if os.path.exists(path):
        embeddings = np.load(path)
        return embeddings
    if feature_fn is None:
        raise RuntimeError('prd_from_image_folders needs --inject feature_fn=dotted.name: the reference\'s '
                           'precision-recall-distributions/inception.pb is not available in this tree')
    imgs = load_images_from_dir(directory)
    embeddings = generate_embedding(imgs, feature_fn, batch_size)
    if not os.path.exists(cache_dir):
        os.makedirs(cache_dir)
    with open(path, 'wb') as f:
        np.save(f, embeddings)
    return embeddings


def main(argv=None):
    from . import dnnlib
    args = build_parser().parse_args(argv)
    if len(args.eval_dirs) != len(args.eval_labels):
        raise ValueError(
            'Number of --eval_dirs must be equal to number of --eval_labels.')
    inject = {key: dnnlib.util.get_obj_by_name(name) for key, name in (args.inject or [])}
    feature_fn = inject.get('feature_fn')
    if args.plot_path is not None or args.inception_path != build_parser().get_default('inception_path'):
        print('note: --plot_path and --inception_path are accepted and ignored (no plot; the embedding network is --inject feature_fn=...)')

    reference_dir = os.path.abspath(args.reference_dir)
    eval_dirs = [os.path.abspath(directory) for directory in args.eval_dirs]

    if args.verbose:
        print('computing inception embeddings for ' + reference_dir)
    real_embeddings = load_or_generate_embedding(reference_dir, args.cache_dir, feature_fn, args.batch_size)
    prd_data = []
    for directory in eval_dirs:
        if args.verbose:
            print('computing inception embeddings for ' + directory)
        eval_embeddings = load_or_generate_embedding(directory, args.cache_dir, feature_fn, args.batch_size)
        if args.verbose:
            print('computing PRD')
        prd_data.append(prd.compute_prd_from_embedding(
            eval_data=eval_embeddings,
            ref_data=real_embeddings,
            num_clusters=args.num_clusters,
            num_angles=args.num_angles,
            num_runs=args.num_runs,
            seed=args.seed))

    print()
    f_beta_data = [prd.prd_to_max_f_beta_pair(precision, recall, beta=8)
                   for precision, recall in prd_data]
    print('F_1/8 (precision)     F_8 (recall)   model')
    for directory, f_beta in zip(eval_dirs, f_beta_data):
        print('%.4f                %.4f         %s' % (f_beta[1], f_beta[0], directory))
    return f_beta_data


if __name__ == '__main__':
    main()
