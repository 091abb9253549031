"""Measured record of the differentiable augmentation (csrc/diffaugment.hip, training/augment.py) -> profiles/augment.txt.

(a) The kernel against the torch statement of the same transform, forward and backward, at [12, 3, 128, 128] (D's step at minibatch_gpu 6: 12 fakes,
    12 reals, one call each) and [6, 3, 128, 128] (G's adversarial term), for the full policy and each single policy:
      ours        device events around `--calls` back-to-back calls of the C entry (igan_diffaugment_fwd / _bwd) on preallocated buffers
      torch       device events around the same number of calls of augment.diffaugment_torch, and around its autograd backward
                  (torch.autograd.grad of the forward's output; the forwards that build the graphs are outside the events)
    after a warm-up of `--warm` seconds of each (the device leaves its idle clock only under load), in `--windows` alternated windows;
    the median window is reported.  Bytes moved = what the algorithm needs: read + write of the batch (colour reads it twice).
    Launches per call come from the profiler (torch.profiler's device activity records) in a pass of its own: `--launches`.
(b) Time per iteration of training_loop() at bench.py's configuration (config-e-Gskip-Dresnet, 128 x 128, minibatch_gpu 6, hipGraphs
    on, NN_rec_lpips_weight 2.5, lazy regularisation) with the full policy against THE SAME COMMIT with the policy off -- the policy-off
    run is the parent commit's path: no draw, no launch -- alternated, `--steps` iterations after `--warmup`, data size `--data-size`.

What this does not measure: the effect of the policy on FID / recall for real CelebA-30k (there is no data in this tree).

    python tools/augment_bench.py [--calls 2000] [--windows 5] [--steps 200] [--warmup 40] [--pairs 2] [--out profiles/augment.txt]
    python tools/augment_bench.py --launches [--out profiles/augment.txt]        (appends)"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import inclusivegan_amd  # noqa: E402,F401 -- first: sets the HIP runtime flags the captured graphs need
import torch  # noqa: E402

from inclusivegan_amd import _abi, hip_ops  # noqa: E402
from inclusivegan_amd.training import augment as A  # noqa: E402

SHAPES = [(12, 3, 128, 128), (6, 3, 128, 128)]
POLICIES = [7, 1, 2, 4]
FULL = 'color,translation,cutout'


def sides(shape, bits, dev):
    """The four timed callables of one configuration: ours forward, ours backward, torch forward, torch backward (the last takes the
    forward output it differentiates)."""
    lib = _abi.get_plugin()
    n, c, h, w = shape
    gen = torch.Generator(device=dev).manual_seed(1)
    x = (torch.rand(shape, device=dev, generator=gen) * 2 - 1).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(shape, device=dev, generator=gen).contiguous(memory_format=torch.channels_last)
    u = torch.rand((n, 8), device=dev, generator=gen)
    y = torch.empty_like(x)
    ws = torch.empty((lib.igan_diffaugment_workspace_bytes(n, c, h, w) // 8,), device=dev, dtype=torch.float64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ours_fwd():
        _abi.check(lib.igan_diffaugment_fwd(stream(), p(x), p(y), p(u), n, c, h, w, bits, p(ws)))

    def ours_bwd():
        _abi.check(lib.igan_diffaugment_bwd(stream(), p(dy), p(y), p(u), n, c, h, w, bits, p(ws)))

    xr = x.clone().requires_grad_(True)

    def torch_fwd():
        with torch.no_grad():
            return A.diffaugment_torch(x, u, bits)

    def torch_graph():
        return A.diffaugment_torch(xr, u, bits)

    def torch_bwd(out):
        return torch.autograd.grad(out, [xr], dy)

    # the two sides compute the same thing at this size (the tests hold both to the fp64 contract)
    hip_y = hip_ops.diffaugment_raw(x, u, bits)
    err = float((hip_y - torch_fwd()).abs().max())
    return dict(ours_fwd=ours_fwd, ours_bwd=ours_bwd, torch_fwd=torch_fwd, torch_graph=torch_graph, torch_bwd=torch_bwd, max_abs_diff=err)


def window(fn, calls, prepare=None):
    """Device time per call over `calls` back-to-back calls, from events on the launch stream."""
    if prepare is None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls
    total = 0.0
    for first in range(0, calls, 50):       # graphs are built outside the events, 50 at a time
        outs = [prepare() for _ in range(min(50, calls - first))]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for o in outs:
            fn(o)
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1) * 1e3
    return total / calls


def warm(fn, seconds):
    t0 = time.time()
    while time.time() - t0 < seconds:
        for _ in range(50):
            fn()
        torch.cuda.synchronize()


def kernel_part(a, emit, dev):
    emit('(a) kernel against the torch statement; us per call, median of %d alternated windows of %d calls (min .. max), after %.1f s of warm-up per side; '
         'GB/s = algorithmic bytes (read + write of the batch; with color the batch is read twice) over that time' % (a.windows, a.calls, a.warm))
    verdict = []
    for shape in SHAPES:
        numel = shape[0] * shape[1] * shape[2] * shape[3]
        for bits in POLICIES:
            s = sides(shape, bits, dev)
            by = numel * 4 * (3 if bits & 1 else 2)
            runs = [('ours forward', lambda: window(s['ours_fwd'], a.calls)), ('torch forward', lambda: window(s['torch_fwd'], a.calls)),
                    ('ours backward', lambda: window(s['ours_bwd'], a.calls)), ('torch backward', lambda: window(s['torch_bwd'], a.calls, s['torch_graph']))]
            warm(s['ours_fwd'], a.warm); warm(s['torch_fwd'], a.warm)
            per = {name: [] for name, _ in runs}
            for _ in range(a.windows):
                for name, run in runs:
                    per[name].append(run())
            emit('%s %-26s max |ours - torch| = %.2e' % (list(shape), ','.join(A.policy_names(bits)), s['max_abs_diff']))
            for name, _ in runs:
                v = per[name]
                med = statistics.median(v)
                emit('    %-15s %8.2f us (%.2f .. %.2f)   %7.1f GB/s' % (name, med, min(v), max(v), by / med / 1e3))
            for d in ('forward', 'backward'):
                o, t = statistics.median(per['ours ' + d]), statistics.median(per['torch ' + d])
                verdict.append(o <= t)
                emit('    %-15s torch / ours = %.2f' % (d + ':', t / o))
    emit('ours is not slower than the torch statement in %d of %d rows' % (sum(verdict), len(verdict)))


def launches_part(a, emit, dev):
    """Kernel launches per call as the profiler records them (device-side kernel activity; copies are listed apart)."""
    from torch.profiler import ProfilerActivity, profile
    emit('launches per call, from the profiler (torch.profiler device activity; kernels / memcpy+memset), one call of each after a warm-up call:')

    def count(fn, prepare=None):
        """fn(prepare()) once untraced, then once under the profiler; what prepare() launches is outside the trace."""
        arg = () if prepare is None else (prepare(),)
        fn(*arg); torch.cuda.synchronize()
        arg = () if prepare is None else (prepare(),)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn(*arg)
            torch.cuda.synchronize()
        dev_events = [e for e in prof.events() if str(e.device_type).endswith('CUDA')]
        copies = [e for e in dev_events if 'memcpy' in e.name.lower() or 'memset' in e.name.lower()]
        return len(dev_events) - len(copies), len(copies), sorted({e.name[:60] for e in dev_events if e not in copies})

    for shape in SHAPES:
        for bits in POLICIES:
            s = sides(shape, bits, dev)
            out = {'ours forward': count(s['ours_fwd']), 'ours backward': count(s['ours_bwd']), 'torch forward': count(s['torch_fwd']),
                   'torch backward': count(s['torch_bwd'], s['torch_graph'])}      # one backward per autograd graph
            emit('%s %-26s %s' % (list(shape), ','.join(A.policy_names(bits)), '   '.join('%s %d / %d' % (k, v[0], v[1]) for k, v in out.items())))
            if bits == 7 and shape == SHAPES[0]:
                emit('    ours forward kernels: %s' % '; '.join(out['ours forward'][2]))
            if out['ours forward'][0] == 0:
                emit('    the profiler recorded no device activity on this box: launch counts NOT measured')
                return


def loop_part(a, emit, dev):
    from inclusivegan_amd.dnnlib import EasyDict
    from inclusivegan_amd.training import training_loop as TL
    B = 6
    data_size = a.data_size // (2 * B) * (2 * B)

    def one(policy):
        state = dict(iters=0, t0=None, t1=None, graphs=None)

        def on_iteration(info):
            state['iters'] += 1
            if state['iters'] == a.warmup:
                info['drain'](); torch.cuda.synchronize()
                state['t0'] = time.perf_counter()
            if state['iters'] == a.warmup + a.steps:
                info['drain'](); torch.cuda.synchronize()
                state['t1'] = time.perf_counter()
                return True
            return False
        extra = {} if policy is None else dict(augment=policy)
        kwargs = dict(            # bench.py's workload
            G_args=EasyDict(func_name='training.networks_stylegan2.G_main', init_mul=1.0, fmap_base=8 << 10, architecture='skip'),
            D_args=EasyDict(func_name='training.networks_stylegan2.D_stylegan2_feature', fmap_base=8 << 10, architecture='resnet'),
            G_opt_args=EasyDict(beta1=0.0, beta2=0.99, epsilon=1e-8), D_opt_args=EasyDict(beta1=0.0, beta2=0.99, epsilon=1e-8),
            G_loss_args=EasyDict(func_name='training.loss.G_logistic_ns_rec_interp_arb_pathreg', NN_rec_lpips_weight=2.5, **extra),
            D_loss_args=EasyDict(func_name='training.loss.D_logistic_r1', gamma=100, **extra),
            dataset_args=EasyDict(resolution=128, num_channels=3, label_size=40, label_kind='attributes'),
            sched_args=EasyDict(G_lrate_base=0.002, D_lrate_base=0.002, minibatch_gpu_base=B, minibatch_size_base=B),
            tf_config={'rnd.np_random_seed': 1000}, total_kimg=10 ** 6, data_size=data_size, num_epochs=10000,
            init_staleness=10, num_samples_factor=10, knn_perturb_factor=0.05, candidate_batch_size=256,
            hooks=dict(on_iteration=on_iteration, on_graphs=lambda g: state.__setitem__('graphs', g), async_ok=True))
        import contextlib
        with contextlib.redirect_stdout(sys.stderr):
            TL.training_loop(**kwargs)
        g = state['graphs'] or {}
        return (state['t1'] - state['t0']) * 1e3 / a.steps, bool(g.get('captured')), bool(g.get('faithful'))

    emit('(b) training_loop() at bench.py\'s configuration (config-e-Gskip-Dresnet, 128 x 128, minibatch_gpu 6, NN_rec_lpips_weight 2.5, lazy regularisation, '
         'hipGraphs on, data size %d, one GPU): ms per iteration over %d iterations after %d of warm-up, host clock around a drained and synchronised window; '
         'policy off = this commit without the flag, which is the parent commit\'s path (no draw, no launch); runs alternated' % (data_size, a.steps, a.warmup))
    res = {None: [], FULL: []}
    for k in range(a.pairs):
        for policy in (None, FULL):
            ms, captured, faithful = one(policy)
            res[policy].append(ms)
            emit('    run %d  policy %-26s %8.3f ms per iteration   (graphs captured %s, faithful %s)' % (k, policy or 'off', ms, captured, faithful))
    off, on = statistics.median(res[None]), statistics.median(res[FULL])
    emit('    median off %.3f ms, median on %.3f ms: the full policy costs %+.3f ms per iteration (%+.2f %%); spread of the off runs %.3f ms'
         % (off, on, on - off, 100 * (on - off) / off, max(res[None]) - min(res[None])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=2000)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--warm', type=float, default=0.5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--pairs', type=int, default=2)
    ap.add_argument('--data-size', type=int, default=1152, help='as the sustained lines of bench.py')
    ap.add_argument('--launches', action='store_true', help='only count the launches per call with the profiler (a pass of its own); appends to --out')
    ap.add_argument('--skip-loop', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda', 0)
    from inclusivegan_amd import hostaffinity
    hostaffinity.limit_host_threads()           # as bench.py: graph replays are host submissions, and a wide OpenMP pool starves them
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if a.launches:
        launches_part(a, emit, dev)
    else:
        emit('augment_bench on %s, torch %s' % (torch.cuda.get_device_properties(0).gcnArchName, torch.__version__))
        kernel_part(a, emit, dev)
        if not a.skip_loop:
            loop_part(a, emit, dev)
        emit('not measured: the effect of the policy on FID / precision / recall for real CelebA-30k (no data in this tree); more than one GPU')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a' if a.launches else 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
