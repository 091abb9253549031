"""The convolution library's dispatch equals the recorded one (tests/golden/conv_dispatch_golden.json).

choose_fwd() / choose_wgrad() in csrc/conv2d_mfma.hip are the one place that picks a kernel; the plan, the kernel-name and the
launch entry points all consume them.  The fixture was recorded from the library BEFORE that change, so equality here says the
refactor moved no shape to another kernel, tile, wave count or plan -- for every convolution of the bench configuration, the
shapes of test_gpu_planes_variant.py and the edge cases listed in tests/golden/make_conv_dispatch_golden.py, under each value of
IGAN_CONV_PLANES and with IGAN_F16_W4=0.  Host-only: no device is touched.
"""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))

_spec = importlib.util.spec_from_file_location('make_conv_dispatch_golden', os.path.join(HERE, 'golden', 'make_conv_dispatch_golden.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def test_dispatch_equals_the_recorded_one():
    want = gen.load()
    got = gen.collect()
    assert got['cases'] == want['cases'], 'the case list changed: regenerate the fixture from a library whose dispatch is known good'
    assert sorted(got['results']) == sorted(want['results'])
    wrong = []
    for env in sorted(want['results']):
        assert len(got['results'][env]) == len(want['cases'])
        for c, g, w in zip(want['cases'], got['results'][env], want['results'][env]):
            if g != w:
                wrong.append((env, c, g, w))
    assert not wrong, '%d answers differ; the first: env %s case %s\n  got  %s\n  want %s' % ((len(wrong),) + wrong[0])


def test_fixture_covers_every_family_and_the_stated_edges():
    want = gen.load()
    names = {env: {r['name'].split('<')[0] for r in res} for env, res in want['results'].items()}
    assert {'dense_small_kernel', 'thin_out_kernel', 'thin_in_kernel', 'conv_fwd_planes_w4_kernel', 'conv_fwd_dma_kernel', 'conv_fwd_kernel',
            'dense_small_wgrad_kernel', 'thin_wgrad_kernel', 'conv_wgrad_planes_kernel', 'conv_wgrad_kernel'} <= names['default']
    assert 'conv_fwd_planes_kernel' in names['IGAN_F16_W4=0'] and 'conv_fwd_planes_kernel' in names['IGAN_CONV_PLANES=1']
    assert not any(n.startswith('conv_fwd_planes') or n == 'conv_wgrad_planes_kernel' for n in names['IGAN_CONV_PLANES=0'])
    assert want['results']['default'] == want['results']['IGAN_CONV_PLANES=2']
    full = {r['name'] for r in want['results']['default']}
    # every fp32 tile shape, and a scalar-load (vec = false) instantiation
    for tile in ('128, 128, 2, 4', '128, 64, 4, 2', '128, 32, 4, 1', '32, 128, 1, 4'):
        assert any(n.startswith('conv_fwd_kernel<%s,' % tile) for n in full), tile
    assert any(n.startswith('conv_fwd_kernel<') and n.split(', ')[5] == 'false' for n in full)
    # the row threshold of the piece form: 1023 rows stay on fp32, 1024 take it
    by_rows = {}
    for c, r in zip(want['cases'], want['results']['default']):
        if c['kind'] == 'fwd' and c['Cin'] == 512 and c['Cout'] == 512 and c['k'] == 3 and not c['in_scale'] and c['x'] % 16 == 0:
            by_rows[c['N'] * c['OH'] * c['OW']] = r['name']
    assert not by_rows[1023].startswith('conv_fwd_planes') and by_rows[1024].startswith('conv_fwd_planes'), by_rows
    # rejected geometries keep their error classes
    assert sorted({r['plan_rc'] for r in want['results']['default']}) == [0, 1, 3]
