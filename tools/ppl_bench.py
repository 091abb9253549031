"""Measured record of the perceptual path length metric (ppl_zfull .. ppl2_wend) on the HIP path.

speed   At the metric's own shape (CelebA-128 config-e G: skip architecture, fmap_base 8192; minibatch_per_gpu 4; 64 x 64
        crop) a window of --window minibatches of PPL's own step is timed after warm-up, alternating in one process with the
        same loop whose new parts are swapped for a torch formulation on the same G and VGG path: tfutil.lerp / tfutil.slerp in
        fp32, slicing, avg_pool2d, the affine, de-interleaving copies and the LPIPS network called on the two image halves, as
        the reference writes it.  Reported: pairs/s and the time 50 000 samples would take.
error   Per-pair relative error of the whole chain against the fp64 CPU oracle at the size of the GPU test (res-32 skip G,
        fmap_base 512, 8 pairs, epsilon 1e-4 and 1e-2, the five space / sampling / crop cases), next to what a plain fp32
        evaluation of the same oracle loses, for the three convolution forms (IGAN_CONV_PLANES unset, 1, 0), each in a
        fresh child process.  The restatement is tests/ppl_oracle.py, the one the GPU test uses, so the record and the test cannot drift.

    python tools/ppl_bench.py [--mode speed|error|both] [--window 64] [--reps 3] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from inclusivegan_amd.dnnlib import tflib                                          # noqa: E402
from inclusivegan_amd.dnnlib.tflib import tfutil                                   # noqa: E402
from inclusivegan_amd.metrics import lpips as lpips_mod                            # noqa: E402
from inclusivegan_amd.metrics.metric_defaults import metric_defaults               # noqa: E402
from inclusivegan_amd.metrics.perceptual_path_length import PPL                    # noqa: E402

G_FUNC = 'inclusivegan_amd.training.networks_stylegan2.G_main'
LPIPS_FUNC = 'inclusivegan_amd.metrics.lpips.vgg16_zhang_perceptual'
CASES = [('w', 'full', True), ('w', 'end', True), ('z', 'full', True), ('z', 'end', True), ('w', 'end', False)]


def torch_minibatch(metric, st):
    """PPL._minibatch with the new kernels swapped for the reference's formulation in torch ops."""
    lat_t01, lerp_t, labels = metric._draw(st)
    if metric.space == 'w':
        dlat_t01 = st.mapping.get_output_for(lat_t01, labels, **st.Gs_kwargs).to(torch.float32)
        dlat_t0, dlat_t1 = dlat_t01[0::2], dlat_t01[1::2]
        dlat_e0 = tfutil.lerp(dlat_t0, dlat_t1, lerp_t[:, None, None])
        dlat_e1 = tfutil.lerp(dlat_t0, dlat_t1, lerp_t[:, None, None] + metric.epsilon)
        dlat_e01 = torch.stack([dlat_e0, dlat_e1], dim=1).reshape(dlat_t01.shape)
    else:
        lat_t0, lat_t1 = lat_t01[0::2], lat_t01[1::2]
        lat_e0 = tfutil.slerp(lat_t0, lat_t1, lerp_t[:, None])
        lat_e1 = tfutil.slerp(lat_t0, lat_t1, lerp_t[:, None] + metric.epsilon)
        lat_e01 = torch.stack([lat_e0, lat_e1], dim=1).reshape(lat_t01.shape)
        dlat_e01 = st.mapping.get_output_for(lat_e01, labels, **st.Gs_kwargs)
    images = st.synthesis.get_output_for(dlat_e01, **st.synthesis_kwargs).to(torch.float32)
    y0, y1, x0, x1 = st.window
    images = images[:, :, y0:y1, x0:x1]
    if st.factor > 1:
        images = torch.nn.functional.avg_pool2d(images, st.factor, st.factor)
    images = (images + 1) * (255 / 2)
    img_e0, img_e1 = images[0::2].contiguous(memory_format=torch.channels_last), images[1::2].contiguous(memory_format=torch.channels_last)
    return st.lpips.get_output_for(img_e0, img_e1) * (1 / metric.epsilon ** 2)


def window(fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        d = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, d


def speed(a, lines):
    dev = torch.device('cuda', 0)
    torch.manual_seed(50003)
    Gs = tflib.Network('Gs', func_name=G_FUNC, architecture='skip', seed=1001, num_channels=3, resolution=a.resolution, label_size=0,
                       fmap_base=8 << 10, device=dev)
    lines.append('ppl_bench speed: G res %d skip fmap_base 8192, minibatch 4 pairs (8 images), window %d minibatches, warm-up %d  (%s)'
                 % (a.resolution, a.window, a.warmup, torch.cuda.get_device_name(0)))
    lines.append('%-10s %-34s %-34s %-10s %-22s' % ('metric', 'HIP step, s per window', 'torch formulation, s per window', 'pairs/s', '50 000 samples, s'))
    for name in a.metrics:
        args = dict(metric_defaults[name])
        metric = PPL(**{k: v for k, v in args.items() if k != 'func_name'})
        with torch.no_grad():
            st = metric._setup(Gs, dict(is_validation=True), 1)
            forms = (('hip', lambda: metric._minibatch(st)), ('torch', lambda: torch_minibatch(metric, st)))
            for _, fn in forms:
                window(fn, a.warmup)
            times = {'hip': [], 'torch': []}
            last = {}
            for _rep in range(a.reps):
                for form, fn in forms:
                    t, last[form] = window(fn, a.window)
                    times[form].append(t)
        best = {k: min(v) for k, v in times.items()}
        per_mb = best['hip'] / a.window
        lines.append('%-10s %-34s %-34s %-10.1f %-22s' % (name, ' '.join('%.3f' % t for t in times['hip']), ' '.join('%.3f' % t for t in times['torch']),
                                                        st.m / per_mb, 'HIP %.0f  torch %.0f' % (per_mb * 50000 / st.m, best['torch'] / a.window * 50000 / st.m)))
        lines.append('%-10s last window\'s distances (different draws): HIP mean %.4g  torch mean %.4g' % ('', float(last['hip'].mean()), float(last['torch'].mean())))
        print('\n'.join(lines[-2:]), flush=True)


def error_child(a):
    from tests import ppl_oracle as T
    dev = torch.device('cuda', 0)
    torch.manual_seed(20261002)
    Gs = tflib.Network('Gs', func_name=G_FUNC, architecture='skip', seed=1, num_channels=3, resolution=T.RES, label_size=0, fmap_base=T.FMAP_BASE, device=dev)
    with torch.no_grad():
        for n, v in Gs.vars.items():
            if n.endswith('noise_strength'):
                v.fill_(0.1)
    lp = {r: tflib.Network('lpips', func_name=LPIPS_FUNC, resolution=r, device=dev, seed=1003) for r in (16, 32)}
    for eps in (1e-4, 1e-2):
        for space, sampling, crop in CASES:
            net = lp[16 if crop else 32]
            metric = PPL(num_samples=8, epsilon=eps, space=space, sampling=sampling, crop=crop, minibatch_per_gpu=4,
                         Gs_overrides=dict(dtype='float32', mapping_dtype='float32'), lpips_net=net, name='ppl')
            rec = tfutil.RecordingRandom()
            with tfutil.use_random(rec):
                d = metric.distances(Gs).astype(np.float64)
            gp = {n: v.detach().double().cpu() for n, v in Gs.vars.items()}
            lpp = {n: v.detach().double().cpu() for n, v in net.vars.items()}
            d64 = T.oracle_distances(rec.entries, gp, lpp, space, crop, eps, 4, torch.float64)
            d32 = T.oracle_distances(rec.entries, gp, lpp, space, crop, eps, 4, torch.float32)
            e32, eh = np.abs(d32 - d64) / d64, np.abs(d - d64) / d64
            print('RESULT eps %-6g %s/%-4s crop=%-5s  fp32 oracle max %.3e   HIP max %.3e  median %.3e   ratio %.3f'
                  % (eps, space, sampling, crop, e32.max(), eh.max(), np.median(eh), eh.max() / e32.max()), flush=True)


def error(a, lines):
    lines.append('ppl_bench error: per-pair relative error against the fp64 oracle, 8 pairs per case; ratio = HIP max / fp32 oracle max')
    for form in (None, '1', '0'):
        env = dict(os.environ)
        env.pop('IGAN_CONV_PLANES', None)
        if form is not None:
            env['IGAN_CONV_PLANES'] = form
        lines.append('IGAN_CONV_PLANES %s' % ('unset' if form is None else '= ' + form))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), '--mode', 'error-child'], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True, timeout=a.child_timeout)
        got = [ln[len('RESULT '):] for ln in out.stdout.splitlines() if ln.startswith('RESULT ')]
        if out.returncode != 0 or len(got) != 2 * len(CASES):
            lines.append('  child failed with status %d:\n%s' % (out.returncode, out.stdout[-2000:]))
            print(lines[-1], flush=True)
            return False
        lines.extend('  ' + ln for ln in got)
        lines.append('  largest ratio %.3f' % max(float(ln.rsplit('ratio', 1)[1]) for ln in got))
        print('\n'.join(lines[-len(got) - 2:]), flush=True)
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', default='both', choices=['speed', 'error', 'both', 'error-child'])
    ap.add_argument('--resolution', type=int, default=128)
    ap.add_argument('--window', type=int, default=64)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--metrics', nargs='+', default=['ppl_wend', 'ppl_zfull'])
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.mode == 'error-child':
        return error_child(a)
    if not torch.cuda.is_available():
        raise SystemExit('ppl_bench needs a ROCm device: nothing is measured without one')
    lines = []
    ok = True
    if a.mode in ('error', 'both'):      # children first: this process has not opened the device yet
        ok = error(a, lines)
    if ok and a.mode in ('speed', 'both'):
        speed(a, lines)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    if not ok:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
