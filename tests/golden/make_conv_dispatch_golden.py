"""Dispatch of the convolution library, recorded: which kernel and which plan every shape gets.

    python tests/golden/make_conv_dispatch_golden.py            # rewrites conv_dispatch_golden.json from the library in the tree

The fixture was written once from a library built BEFORE choose_fwd() / choose_wgrad() replaced the duplicated decisions of
igan_conv2d / igan_conv2d_kernel_name (and their weight-gradient twins); tests/test_conv_dispatch_golden.py asserts that the
library in the tree still answers the same.  Regenerate it only with a change that means to move the dispatch.

Everything here is host-only: igan_conv2d_plan, igan_conv2d_kernel_name and the two wgrad entry points never touch a device
(without one the library plans for 256 CUs, the MI355X's), and the pointers are made-up integers that nothing dereferences.
The library reads its switches once, so every environment runs in a child process of its own.
"""
import ctypes
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, 'conv_dispatch_golden.json')
SHAPES = os.path.join(ROOT, 'profiles', 'r06_conv_shapes.txt')

ENVS = {
    'default': {},
    'IGAN_CONV_PLANES=0': {'IGAN_CONV_PLANES': '0'},
    'IGAN_CONV_PLANES=1': {'IGAN_CONV_PLANES': '1'},
    'IGAN_CONV_PLANES=2': {'IGAN_CONV_PLANES': '2'},
    'IGAN_F16_W4=0': {'IGAN_F16_W4': '0'},
}
# fake operand addresses: 16-byte aligned, apart, never dereferenced
X, W_, Y, S_IN, S_OUT, BIAS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000


def case(kind, N, H, W, Cin, OH, OW, Cout, k, stride=1, up=1, pad=None, in_scale=False, out_scale=False, act=0, x=X):
    """kind: 'fwd', 'dgrad' (a forward-type call with the filter transposed) or 'wgrad'."""
    if pad is None:     # the smallest symmetric padding that gives OH from H (what every layer of the networks uses)
        U = (H - 1) * up + 1
        pad = next(p for p in range(0, 2 * k + 2) if (U + 2 * p - k) // stride + 1 == OH)
    return dict(kind=kind, N=N, H=H, W=W, Cin=Cin, OH=OH, OW=OW, Cout=Cout, k=k, stride=stride, up=up, pad=pad,
                in_scale=bool(in_scale), out_scale=bool(out_scale), act=int(act), x=x)


LINE = re.compile(r'^(fwd|dgrad|wgrad)(\+scale)?(\+act)?\s+N(\d+)\s+(\d+)x(\d+)\s+C(\d+)\s+->\s+(\d+)x(\d+)\s+C(\d+)\s+k(\d+) s(\d+) u(\d+) splits')


def bench_cases():
    """Every convolution and weight-gradient shape of the bench configuration (profiles/r06_conv_shapes.txt)."""
    out = []
    with open(SHAPES) as fh:
        for ln in fh:
            m = LINE.match(ln)
            if not m:
                assert ln.startswith('#') or not ln.strip(), ln
                continue
            kind, sc, act = m.group(1), m.group(2) is not None, m.group(3) is not None
            N, H, W, Cin, OH, OW, Cout, k, s, u = (int(v) for v in m.groups()[3:])
            # '+scale' says that a scale operand was passed, not which: both (a demodulated layer) and the input's alone (ToRGB)
            for both in ((True, False) if sc else (False,)):
                out.append(case(kind, N, H, W, Cin, OH, OW, Cout, k, s, u, in_scale=sc, out_scale=both, act=3 if act else 0))
    return out


def edge_cases():
    out = []
    # tests/test_gpu_planes_variant.py: the piece-form shapes, the shapes it leaves to fp32, its weight gradients, its digest shape
    for N, Cin, H, Cout, k, s, u, pad, o, sc in ((3, 256, 32, 256, 3, 1, 1, 1, 32, True), (9, 512, 16, 512, 3, 1, 1, 1, 16, False),
                                                 (9, 256, 33, 512, 3, 2, 1, 0, 16, False), (8, 512, 16, 256, 3, 1, 2, 2, 33, True),
                                                 (4, 128, 24, 384, 3, 1, 1, 1, 24, False), (24, 512, 8, 512, 3, 1, 1, 1, 8, True),
                                                 (2, 128, 64, 256, 1, 1, 1, 0, 64, False), (2, 64, 32, 128, 3, 1, 1, 1, 32, False),
                                                 (3, 512, 8, 512, 3, 1, 1, 1, 8, False), (4, 256, 32, 256, 3, 1, 1, 1, 32, True),
                                                 (6, 160, 19, 224, 3, 1, 1, 1, 19, False)):      # the last: ragged channel counts
        for kind in ('fwd', 'dgrad', 'wgrad'):
            out.append(case(kind, N, H, H, Cin, o, o, Cout, k, s, u, pad, in_scale=sc, out_scale=sc))
    for kind in ('fwd', 'dgrad', 'wgrad'):
        for Cout in (32, 64):                                                   # the narrow tiles
            out.append(case(kind, 4, 32, 32, 128, 32, 32, Cout, 3))
            out.append(case(kind, 4, 32, 32, Cout, 32, 32, 128, 3))
        out.append(case(kind, 2, 4, 4, 512, 4, 4, 512, 3))                     # Mmax <= 32 with Cout > 64: the 32-row tile
        out.append(case(kind, 2, 4, 4, 512, 4, 4, 512, 3, in_scale=True))      # ... and exactly one scale
        out.append(case(kind, 8, 1, 1, 512, 1, 1, 512, 1))                     # 1x1 on a 1x1 map: the small dense path
        out.append(case(kind, 64, 1, 1, 512, 1, 1, 512, 1))                    # ... with too many rows for it
        out.append(case(kind, 4, 32, 32, 3, 32, 32, 3, 1))                     # thin: three channels on each side
        out.append(case(kind, 4, 32, 32, 3, 32, 32, 3, 3))
        out.append(case(kind, 4, 32, 32, 256, 32, 32, 3, 1))                   # ToRGB-shaped
        out.append(case(kind, 3, 11, 31, 512, 11, 31, 512, 3))                 # 1023 rows: below the piece form's threshold
        out.append(case(kind, 1, 32, 32, 512, 32, 32, 512, 3))                 # 1024 rows: at it
        out.append(case(kind, 4, 32, 32, 64, 32, 32, 64, 3, x=20))             # x misaligned by 4: the scalar-load instantiations
        out.append(case(kind, 4, 32, 32, 256, 32, 32, 256, 3, x=20))           # ... on a shape that would take the piece form
        out.append(case(kind, 4, 128, 128, 128, 128, 128, 128, 3, pad=1))      # a long pixel axis (the weight gradient's four-wave tile)
    out.append(case('fwd', 4, 32, 32, 256, 32, 32, 256, 3, stride=1, up=3, pad=1))     # rejected: up must be 1 or 2
    out.append(case('wgrad', 4, 32, 32, 256, 32, 32, 256, 3, stride=2, up=2, pad=1))   # rejected: stride and up together
    return out


def all_cases():
    seen, out = set(), []
    for c in bench_cases() + edge_cases():
        key = json.dumps(c, sort_keys=True)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def query(cases):
    """Ask the library in the tree (this process: its switches are whatever the environment holds)."""
    sys.path.insert(0, ROOT)
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    res = []
    for c in cases:
        common = dict(x=c['x'], in_scale=S_IN if c['in_scale'] else None, out_scale=S_OUT if c['out_scale'] else None, workspace=None, workspace_floats=0,
                      N=c['N'], H=c['H'], W=c['W'], Cin=c['Cin'], OH=c['OH'], OW=c['OW'], Cout=c['Cout'], KH=c['k'], KW=c['k'],
                      stride=c['stride'], up=c['up'], pad_y=c['pad'], pad_x=c['pad'], splits=1, alpha=1.0)
        buf = ctypes.create_string_buffer(160)
        splits, ws = ctypes.c_int(-1), ctypes.c_size_t(0)
        if c['kind'] == 'wgrad':
            p = _abi.Conv2DWgradParams(dy=Y, dw=W_, **common)
            rc = lib.igan_conv2d_wgrad_plan(ctypes.byref(p), ctypes.byref(splits), ctypes.byref(ws))
            r = dict(plan_rc=rc, splits=splits.value, workspace_floats=ws.value)
            r['name_rc'] = lib.igan_conv2d_wgrad_kernel_name(ctypes.byref(p), buf, 160)
        else:
            sliced = ctypes.c_int(-1)
            p = _abi.Conv2DParams(w=W_, y=Y, w_transposed=1 if c['kind'] == 'dgrad' else 0, bias=BIAS if c['act'] else None, act=c['act'],
                                  act_alpha=0.2, act_gain=1.0, **common)
            rc = lib.igan_conv2d_plan(ctypes.byref(p), ctypes.byref(splits), ctypes.byref(sliced), ctypes.byref(ws))
            r = dict(plan_rc=rc, splits=splits.value, sliced_tiles=sliced.value, workspace_floats=ws.value)
            r['name_rc'] = lib.igan_conv2d_kernel_name(ctypes.byref(p), buf, 160)
        r['name'] = buf.value.decode()
        res.append(r)
    return res


def collect():
    """{'cases': [...], 'results': {environment: [one answer per case]}}, every environment in a child process."""
    out = {'cases': all_cases(), 'results': {}}
    for name, extra in ENVS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith('IGAN_') or k == 'IGAN_LIB'}
        env.update(extra)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        out['results'][name] = json.loads(r.stdout)
    return out


# The fixture file: one line per case -- the case, then its answer in every environment of ENVS, in order, as
# "plan_rc name_rc splits sliced_tiles workspace_floats name" (sliced_tiles '-' for a weight gradient); "=" repeats the default's.
KEY = '%(kind)s N%(N)d %(H)dx%(W)d C%(Cin)d -> %(OH)dx%(OW)d C%(Cout)d k%(k)d s%(stride)d u%(up)d pad%(pad)d'
KEY_RE = re.compile(r'^(\w+) N(\d+) (\d+)x(\d+) C(\d+) -> (\d+)x(\d+) C(\d+) k(\d+) s(\d+) u(\d+) pad(\d+)(?: scale(\d)(\d))?(?: act(\d))?(?: x(\d+))?$')


def key(c):     # in_scale / out_scale, act and a made-up x address appear only where they are not none, 0 and X
    return (KEY % c + (' scale%d%d' % (c['in_scale'], c['out_scale']) if c['in_scale'] or c['out_scale'] else '') +
            (' act%d' % c['act'] if c['act'] else '') + (' x%d' % c['x'] if c['x'] != X else ''))


def save(data, path=FIXTURE):
    envs = list(ENVS)
    with open(path, 'w') as fh:
        fh.write('{"environments": %s,\n"cases": [\n' % json.dumps(envs))
        rows = []
        for i, c in enumerate(data['cases']):
            ans = ['%d %d %d %s %d %s' % (r['plan_rc'], r['name_rc'], r['splits'], r.get('sliced_tiles', '-'), r['workspace_floats'], r['name'])
                   for r in (data['results'][e][i] for e in envs)]
            rows.append(json.dumps([key(c)] + [ans[0]] + ['=' if a == ans[0] else a for a in ans[1:]]))
        fh.write(',\n'.join(rows) + '\n]}\n')


def load(path=FIXTURE):
    """The fixture in the form collect() returns."""
    with open(path) as fh:
        raw = json.load(fh)
    assert raw['environments'] == list(ENVS)
    out = {'cases': [], 'results': {e: [] for e in ENVS}}
    for row in raw['cases']:
        g = KEY_RE.match(row[0]).groups()
        v = [int(t) for t in g[1:12]] + [int(g[12] or 0), int(g[13] or 0), int(g[14] or 0), int(g[15]) if g[15] else X]
        out['cases'].append(dict(kind=g[0], N=v[0], H=v[1], W=v[2], Cin=v[3], OH=v[4], OW=v[5], Cout=v[6], k=v[7], stride=v[8], up=v[9], pad=v[10],
                                 in_scale=bool(v[11]), out_scale=bool(v[12]), act=v[13], x=v[14]))
        for e, a in zip(ENVS, row[1:]):
            t = (row[1] if a == '=' else a).split(' ', 5)
            r = dict(plan_rc=int(t[0]), name_rc=int(t[1]), splits=int(t[2]), workspace_floats=int(t[4]), name=t[5])
            if t[3] != '-':
                r['sliced_tiles'] = int(t[3])
            out['results'][e].append(r)
    return out


if __name__ == '__main__':
    if sys.argv[1:] == ['--child']:
        json.dump(query(all_cases()), sys.stdout)
    else:
        save(collect())
        print('wrote %s: %d cases x %d environments' % (FIXTURE, len(all_cases()), len(ENVS)))
