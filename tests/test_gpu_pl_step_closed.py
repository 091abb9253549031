"""GPU: one path-length step at 32x32 (fmap_base 8192, minibatch_gpu 6: path-length batch 3) from ONE saved state, with the style path's closed second-order
Functions (the default) and with the per-layer composites (IGAN_STYLE_CLOSED2=0), each in a child process, each against the fp64 oracle -- the method of
tests/test_gpu_reg_forms.py (tests/reg_forms.py), at pl_mean = 0 and at 0.9 x the batch's mean path length.

Bar: the regulariser's value, pl_mean and every trainable's gradient; per variable the closed form deviates from fp64 by at most 2 x what the composite does,
and both forms sit inside that test's bounds (5e-3 per variable, 1e-3 on the value)."""
import os

import pytest
import torch

from tests import reg_forms as RF

pytestmark = pytest.mark.gpu

FACTOR = 2.0
FORMS = [('composite', '0'), ('closed', '1')]


def test_path_length_step_closed_vs_composite_vs_oracle(cuda_device, tmp_path):
    state, names = RF.init_state(cuda_device, 32, 8192, 6, pl_fracs=(0.0, 0.9))
    torch.cuda.empty_cache()
    spath = str(tmp_path / 'state.npz')
    RF.save_state_dict(spath, state)
    hip = {}
    for label, switch in FORMS:
        opath = str(tmp_path / ('out_%s.npz' % label))
        RF.run_child(spath, opath, dict(IGAN_STYLE_CLOSED2=switch), ops=('G_reg',))
        hip[label] = RF.load_result(opath)
        os.remove(opath)
    ora = RF.oracle_ops_of_state(state, ops=('G_reg',), trainables=names)
    labels = [l for l, _ in FORMS]
    devs = {l: {op: RF.deviations(hip[l][op], ora[op]) for op in ora} for l in labels}
    print(RF.table(devs, labels, top=100))
    bad = []
    for op in ora:
        for l in labels:
            worst = max(devs[l][op]['errs'].values())
            if not worst < 5e-3:
                bad.append('%s %s: worst per-variable deviation %.2e exceeds 5e-3' % (op, l, worst))
            if not devs[l][op]['value'] < 1e-3:
                bad.append('%s %s: value deviation %.2e exceeds 1e-3' % (op, l, devs[l][op]['value']))
            if not devs[l][op]['pl_mean'] < 1e-3:
                bad.append('%s %s: pl_mean deviation %.2e exceeds 1e-3' % (op, l, devs[l][op]['pl_mean']))
        c, p = devs['closed'][op], devs['composite'][op]
        assert set(c['errs']) == set(p['errs'])
        for n in c['errs']:
            if not c['errs'][n] <= FACTOR * p['errs'][n]:
                bad.append('%s %s: closed %.2e > %g x composite %.2e' % (op, n, c['errs'][n], FACTOR, p['errs'][n]))
    assert not bad, '\n'.join(bad)
