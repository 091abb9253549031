"""Golden data for the inference CLIs, produced by EXECUTING the reference's own run_generator.generate_images and the
argument parsers of its run_generator.py / run_metrics.py.

The reference modules import TensorFlow-side packages at module level, so they are loaded from where the reference lies
(/root/reference, read at generation time only; nothing of its text is stored in the repo) with small recording stand-ins
in sys.modules:

    real (reference code)   generate_images (run_generator.py:19-37), both main() functions up to parse_args, NumPy's RandomState
    stand-ins               pretrained_networks.load_networks (a stub Gs: input_shape [None, 8], synthesis variables noise0
                            [1, 1, 4, 4], noise1 [1, 1, 8, 8] and one that is no noise input), tflib.set_vars and Gs.run
                            (record what they are given), PIL.Image (records the file names), dnnlib.make_run_dir_path

Output: tests/golden/generator_golden.npz -- data only: per case and minibatch the z array and the set_vars values by
variable name, the kwargs of Gs.run and the file names as JSON, and each parser's options (flags, dest, default, required).
tests/test_inference_surface.py drives inclusivegan_amd.run_generator / run_metrics against it.

Run from the repo root:  python tests/golden/make_generator_golden.py   (needs /root/reference)
"""
import argparse
import importlib.util
import json
import os
import sys
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
CASES = {'plain': dict(num_images=5, minibatch_size=2), 'psi': dict(num_images=5, minibatch_size=2, truncation_psi=0.5)}


class _Shape:
    def __init__(self, dims):
        self.dims = list(dims)

    def as_list(self):
        return list(self.dims)


class _Var:
    def __init__(self, name, dims):
        self.name, self.shape = name, _Shape(dims)


class EasyDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class Recorder:
    def __init__(self):
        self.z, self.set_vars, self.run_kwargs, self.files = [], [], [], []


def convert_images_to_uint8(*args, **kwargs):
    raise AssertionError('the stand-in Gs.run never calls its transform')


def install_stubs(rec):
    class Synthesis:
        vars = OrderedDict([('noise0', _Var('noise0', [1, 1, 4, 4])), ('4x4/Const/const', _Var('const', [1, 16, 4, 4])),
                            ('noise1', _Var('noise1', [1, 1, 8, 8]))])

    class Gs:
        input_shape = [None, 8]
        components = EasyDict(synthesis=Synthesis)

        @staticmethod
        def run(z, labels, **kwargs):
            assert labels is None
            rec.z.append(np.array(z))
            kw = {k: ({kk: (vv.__name__ if callable(vv) else vv) for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in kwargs.items()}
            rec.run_kwargs.append(kw)
            return np.zeros([z.shape[0], 8, 8, 3], np.uint8)

    class Image:
        def __init__(self, mode):
            self.mode = mode

        def save(self, path):
            rec.files.append([path, self.mode])

    mods = {name: types.ModuleType(name) for name in ('pretrained_networks', 'dnnlib', 'dnnlib.tflib', 'PIL', 'PIL.Image', 'metrics',
                                                      'metrics.metric_base', 'metrics.metric_defaults')}
    mods['pretrained_networks'].load_networks = lambda path: ('G', 'D', Gs)
    mods['dnnlib'].EasyDict = EasyDict
    mods['dnnlib'].make_run_dir_path = lambda name: name
    mods['dnnlib'].tflib = mods['dnnlib.tflib']
    mods['dnnlib.tflib'].convert_images_to_uint8 = convert_images_to_uint8
    mods['dnnlib.tflib'].set_vars = lambda d: rec.set_vars.append({var.name: np.array(value) for var, value in d.items()})
    mods['PIL'].Image = mods['PIL.Image']
    mods['PIL.Image'].fromarray = lambda arr, mode=None: Image(mode)
    mods['metrics'].metric_base = mods['metrics.metric_base']
    mods['metrics.metric_defaults'].metric_defaults = {}
    sys.modules.update(mods)


def load_reference_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Parsed(Exception):
    pass


def parser_options(main):
    """Run main() up to parse_args and list every option of the parser (and of its sub-commands)."""
    seen = []

    def parse_args(self, *a, **k):
        seen.append(self)
        raise _Parsed()

    orig = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = parse_args
    try:
        main()
    except _Parsed:
        pass
    finally:
        argparse.ArgumentParser.parse_args = orig

    def options(parser, prefix):
        rows = []
        for a in parser._actions:
            if isinstance(a, argparse._SubParsersAction):
                for cmd, sub in a.choices.items():
                    rows += options(sub, prefix + cmd + ' ')
            elif a.option_strings and a.dest != 'help':
                rows.append(dict(command=prefix.strip(), flags=list(a.option_strings), dest=a.dest, default=a.default, required=bool(a.required)))
        return rows
    return options(seen[0], '')


def main():
    out = {}
    for case, kw in CASES.items():
        rec = Recorder()
        install_stubs(rec)
        ref = load_reference_module('run_generator')
        stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
        try:
            ref.generate_images('stub.pkl', **kw)
        finally:
            sys.stdout = stdout
        out[case + '/num_minibatches'] = np.int64(len(rec.z))
        for i, z in enumerate(rec.z):
            out['%s/z/%d' % (case, i)] = z
            for name, value in rec.set_vars[i].items():
                out['%s/set_vars/%d/%s' % (case, i, name)] = value
        out[case + '/run_kwargs'] = np.array(json.dumps(rec.run_kwargs, sort_keys=True))
        out[case + '/files'] = np.array(json.dumps(rec.files))
        out[case + '/args'] = np.array(json.dumps(kw, sort_keys=True))
        if case == 'plain':
            out['parse_num_range/3-6'] = np.array(list(ref._parse_num_range('3-6')))
            out['parse_num_range/1,4'] = np.array(list(ref._parse_num_range('1,4')))
            out['parser/run_generator'] = np.array(json.dumps(parser_options(ref.main), sort_keys=True))
            out['parser/run_metrics'] = np.array(json.dumps(parser_options(load_reference_module('run_metrics').main), sort_keys=True))
    np.savez_compressed(os.path.join(HERE, 'generator_golden.npz'), **out)
    for k in ('plain/files', 'plain/run_kwargs', 'psi/run_kwargs', 'parser/run_generator', 'parser/run_metrics'):
        print(k, out[k])


if __name__ == '__main__':
    main()
