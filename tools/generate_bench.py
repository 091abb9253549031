#!/usr/bin/env python3
"""Record of the inference surface on one MI355X: `python tools/generate_bench.py --out profiles/generate_images.txt`.

(a) Device time of igan_images_to_uint8 (hip_ops.images_to_uint8, NCHW fp32 -> NHWC uint8) against the torch chain the metrics
    used before it (scale, + bias, clamp, cast, permuted copy) on the same tensors, [50, 3, 128, 128] and [8, 3, 1024, 1024]:
    device events around `--reps` back-to-back calls, after a warm-up, the two forms alternating, median of `--windows` windows.
    The calls of a window rotate over enough input tensors to exceed the 256 MiB last-level cache at the large size, so that the
    reads come from HBM.  Achieved bytes/s = (4 + 1) bytes per value over the time per call; the share of the 8 TB/s HBM peak is
    printed for the large size only -- at the small one (12 MB in flight, a few microseconds) the launch bounds the time.
(b) Images per second of run_generator.generate_images at 128 x 128 (config-e G, minibatch 50) against the same loop the way it
    had to be written before: Gs.run without transform (fp32 copy-back), the torch conversion on the host tensor, PNG files
    written one after the other.  That older way lives in this tool only.  The split of one minibatch (generate, convert and
    copy, encode) is printed next to it, so that a loop bound by PNG encoding shows as such.

No threshold is attached to the numbers."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12       # bytes/s


def torch_chain(images, nchw_to_nhwc=True):
    """metrics/metric_base.convert_images_to_uint8 as it was before the kernel, on whatever device `images` is on."""
    import torch
    images = images.to(torch.float32)
    if nchw_to_nhwc:
        images = images.permute(0, 2, 3, 1)
    images = images * 127.5 + (0.5 - -1 * 127.5)
    return images.clamp(0, 255).to(torch.uint8).contiguous()


def time_window(fn, inputs, reps):
    """Mean device time of one call in microseconds: events around `reps` back-to-back calls rotating over `inputs`."""
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(reps):
        fn(inputs[i % len(inputs)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def kernel_record(out, shape, reps, windows, warmup):
    import torch
    from inclusivegan_amd import hip_ops
    dev = torch.device('cuda', 0)
    numel = int(np.prod(shape))
    copies = max(2, -(-(320 << 20) // (4 * numel)))             # > 256 MiB of inputs in rotation
    gen = torch.Generator(device=dev).manual_seed(1)
    inputs = [torch.randn(shape, device=dev, generator=gen).clamp_(-1.2, 1.2) for _ in range(copies)]

    def kernel(x):
        return hip_ops.images_to_uint8(x, (-1, 1), True, 1)

    same = all(torch.equal(kernel(x), torch_chain(x)) for x in inputs[:2])
    for _ in range(warmup):
        kernel(inputs[0]); torch_chain(inputs[0])
    torch.cuda.synchronize()
    t_kernel, t_torch = [], []
    for _ in range(windows):
        t_kernel.append(time_window(kernel, inputs, reps))
        t_torch.append(time_window(torch_chain, inputs, reps))
    k, t = float(np.median(t_kernel)), float(np.median(t_torch))
    rate = 5.0 * numel / (k * 1e-6)
    out('  %-20s %d inputs in rotation, %d windows of %d calls; bytes equal to the torch chain: %s' % (list(shape), copies, windows, reps, same))
    out('    kernel   %8.2f us per call (windows %s)' % (k, ' '.join('%.2f' % v for v in t_kernel)))
    out('    torch    %8.2f us per call (windows %s)   kernel / torch = %.3f' % (t, ' '.join('%.2f' % v for v in t_torch), k / t))
    if numel >= 1 << 24:
        out('    kernel moves %.1f MB per call: %.2f TB/s = %.3f of the 8 TB/s HBM peak' % (5.0 * numel / 1e6, rate / 1e12, rate / HBM_PEAK))
    else:
        out('    %.1f MB per call in %.1f us: launch-bound at this size (time per call of back-to-back launches), no share of peak is quoted' % (5.0 * numel / 1e6, k))


def old_generate_images(Gs, num_images, minibatch_size, run_dir, split):
    """The generator loop before output_transform existed: fp32 copy-back, torch conversion on the host, serial PNG writes."""
    import PIL.Image
    import torch
    from inclusivegan_amd.dnnlib import tflib
    noise_vars = [var for name, var in Gs.components.synthesis.vars.items() if name.startswith('noise')]
    rnd = np.random.RandomState(0)
    for image_idx in range(0, num_images, minibatch_size):
        z = rnd.randn(minibatch_size, *Gs.input_shape[1:])
        tflib.set_vars({var: rnd.randn(*[int(s) for s in var.shape]) for var in noise_vars})
        t0 = time.perf_counter()
        images = Gs.run(z, None, randomize_noise=True)
        t1 = time.perf_counter()
        images = torch_chain(torch.from_numpy(images)).numpy()
        t2 = time.perf_counter()
        for i in range(minibatch_size):
            PIL.Image.fromarray(images[i], 'RGB').save(os.path.join(run_dir, '%06d.png' % (image_idx + i)))
        t3 = time.perf_counter()
        split['generate + fp32 copy-back'] += t1 - t0
        split['torch conversion on the host'] += t2 - t1
        split['serial PNG writes'] += t3 - t2


def generator_record(out, num_images, minibatch_size, windows):
    import torch
    from inclusivegan_amd import pretrained_networks, run_generator
    from inclusivegan_amd.dnnlib import tflib
    from inclusivegan_amd.training import misc
    dev = torch.device('cuda', 0)
    kw = dict(num_channels=3, resolution=128, label_size=0, fmap_base=8 << 10, architecture='skip', device=dev)
    Gs = tflib.Network('Gs', func_name='inclusivegan_amd.training.networks_stylegan2.G_main', seed=1, **kw)
    work = tempfile.mkdtemp(prefix='generate_bench_')
    try:
        pkl = os.path.join(work, 'network-snapshot-000000.pkl')
        misc.save_pkl((None, None, Gs), pkl)
        Gs = pretrained_networks.load_networks(pkl)[-1]
        # split of one minibatch on the new path, measured apart from the end-to-end windows
        z = np.random.RandomState(0).randn(minibatch_size, *Gs.input_shape[1:])
        kwargs = dict(output_transform=dict(func=tflib.convert_images_to_uint8, nchw_to_nhwc=True), randomize_noise=True)
        for _ in range(3):
            images = Gs.run(z, None, **kwargs)
        t0 = time.perf_counter()
        for _ in range(5):
            images = Gs.run(z, None, **kwargs)
        t_run = (time.perf_counter() - t0) / 5
        t0 = time.perf_counter()
        for i in range(minibatch_size):
            run_generator._save_png(images[i], os.path.join(work, 'probe.png'))
        t_png = time.perf_counter() - t0

        new, old, splits = [], [], []
        for w in range(windows):
            d = os.path.join(work, 'new%d' % w)
            t0 = time.perf_counter()
            run_generator.generate_images(pkl, num_images, minibatch_size, run_dir=d)
            new.append(num_images / (time.perf_counter() - t0))
            d = os.path.join(work, 'old%d' % w)
            os.makedirs(d)
            split = {'generate + fp32 copy-back': 0.0, 'torch conversion on the host': 0.0, 'serial PNG writes': 0.0}
            t0 = time.perf_counter()
            old_generate_images(Gs, num_images, minibatch_size, d, split)
            old.append(num_images / (time.perf_counter() - t0))
            splits.append(split)
        n_mb = -(-num_images // minibatch_size)
        out('  generate_images, 128 x 128 config-e G, %d images in minibatches of %d, %d alternating windows (first window includes warm-up)' % (num_images, minibatch_size, windows))
        out('    new   %s img/s   best %.1f' % (' '.join('%.1f' % v for v in new), max(new)))
        out('    old   %s img/s   best %.1f   (fp32 copy-back, torch conversion on the host, serial PNG writes)' % (' '.join('%.1f' % v for v in old), max(old)))
        out('    new path, one minibatch: Gs.run with the uint8 NHWC transform %.1f ms; encoding its %d PNGs on ONE thread %.1f ms (%d writer threads share it)'
            % (t_run * 1e3, minibatch_size, t_png * 1e3, run_generator.NUM_PNG_WRITERS))
        last = splits[-1]
        out('    old path, per minibatch (last window): ' + '; '.join('%s %.1f ms' % (k, v / n_mb * 1e3) for k, v in last.items()))
        bound = 'PNG encoding' if t_png / run_generator.NUM_PNG_WRITERS > t_run else 'the generator'
        out('    new path is bound by %s: %.1f ms of encoding per minibatch over %d threads = %.1f ms against %.1f ms of Gs.run'
            % (bound, t_png * 1e3, run_generator.NUM_PNG_WRITERS, t_png * 1e3 / run_generator.NUM_PNG_WRITERS, t_run * 1e3))
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--num-images', type=int, default=500)
    ap.add_argument('--minibatch-size', type=int, default=50)
    ap.add_argument('--generator-windows', type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('generate_bench needs a ROCm device: nothing is measured without one')
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)

    out('generate_bench: `python tools/generate_bench.py%s` on %s' % (' --out ' + args.out if args.out else '', torch.cuda.get_device_name(0)))
    out('(a) images_to_uint8, NCHW fp32 -> NHWC uint8, drange [-1, 1]; device events, %d warm-up calls' % args.warmup)
    for shape in ((50, 3, 128, 128), (8, 3, 1024, 1024)):
        kernel_record(out, shape, args.reps, args.windows, args.warmup)
    out('(b) run_generator.generate_images')
    generator_record(out, args.num_images, args.minibatch_size, args.generator_windows)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
