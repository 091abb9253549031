"""CPU: the pieces of the multi-rank fid30k that need no device -- igan_moments_merge validates its arguments before a device
is touched, MetricBase.run / MetricGroup.run take `process_group=None` and behave as before, the rule that deals the rows of a
global minibatch to the ranks (frechet_inception_distance.shard_slices) tiles [0, num_images), and run_metrics.main refuses
`--num-gpus 2` in a single process with the launcher's command line."""
import numpy as np
import pytest


def test_merge_entry_validates_without_a_device():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    assert lib.igan_abi_version() == _abi.ABI_VERSION == 10          # one more export: no bump
    P = 1 << 20           # never dereferenced: validation fails first
    bad, unsupported = _abi.IGAN_ERR_INVALID_ARGUMENT, _abi.IGAN_ERR_UNSUPPORTED

    def merge(n_b=100, F=64, same_gram=False, same_sum=False, **null):
        sa, ga, sha, sb, gb, shb = (None if b in null else P * (i + 1) for i, b in enumerate(('sum_a', 'gram_a', 'shift_a', 'sum_b', 'gram_b', 'shift_b')))
        return lib.igan_moments_merge(None, sa, ga, sha, sa if same_sum else sb, ga if same_gram else gb, shb, n_b, F)

    assert merge(F=4097) == unsupported and b'F <= 4096' in lib.igan_last_error()
    for F in (0, -1):
        assert merge(F=F) == bad and b'F must be positive' in lib.igan_last_error()
    for n_b in (0, -5):
        assert merge(n_b=n_b) == bad and b'n_b must be positive' in lib.igan_last_error()
    for b in ('sum_a', 'gram_a', 'sum_b', 'gram_b'):
        assert merge(**{b: None}) == bad and b'null buffer' in lib.igan_last_error(), b
    assert merge(same_gram=True) == bad and b'alias' in lib.igan_last_error()
    assert merge(same_sum=True) == bad and b'alias' in lib.igan_last_error()
    with pytest.raises(NotImplementedError):
        _abi.check(merge(F=4097))
    with pytest.raises(ValueError):
        _abi.check(merge(n_b=0))


def test_python_merge_has_no_cpu_path():
    import torch
    from inclusivegan_amd import hip_ops
    s, g = torch.zeros(4, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        hip_ops.moments_merge_raw(s, g, None, s.clone(), g.clone(), None, 3)


def test_run_takes_process_group_none_and_behaves_as_before(tmp_path, capsys):
    import inspect
    from inclusivegan_amd.metrics import metric_base
    assert list(inspect.signature(metric_base.MetricBase.run).parameters)[-1] == 'process_group'
    assert inspect.signature(metric_base.MetricBase.run).parameters['process_group'].default is None
    assert inspect.signature(metric_base.MetricGroup.run).parameters['process_group'].default is None
    assert metric_base.MetricBase.multi_rank is False and metric_base.DummyMetric.multi_rank is False
    from inclusivegan_amd.metrics import frechet_inception_distance as FM
    assert FM.FID.multi_rank is True

    plain, keyed = metric_base.DummyMetric(name='dummy'), metric_base.DummyMetric(name='dummy')
    plain.run(object(), run_dir=str(tmp_path))
    keyed.run(object(), run_dir=str(tmp_path), process_group=None)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 2 and 'dummy 0.0000' in out[0] and 'dummy 0.0000' in out[1]
    assert [r.value for r in keyed._results] == [r.value for r in plain._results] == [0.0]
    with open(str(tmp_path / 'metric-dummy.txt')) as f:
        assert len(f.read().strip().splitlines()) == 2

    group = metric_base.MetricGroup([dict(func_name='inclusivegan_amd.metrics.metric_base.DummyMetric', name='dummy')])
    group.run(object(), log_results=False, process_group=None)
    group.run(object(), log_results=False)
    assert [r.value for r in group.metrics[0]._results] == [0.0]
    assert 'dummy 0.0000' in group.get_result_str()
    # a metric that runs on one rank refuses a group instead of quietly evaluating on every rank
    with pytest.raises(ValueError, match='one rank'):
        plain.run(object(), process_group=object())


@pytest.mark.parametrize('num_images,mb,world,want_counts', [(100, 16, 2, [52, 48]), (30, 16, 2, [16, 14]), (7, 3, 4, [3, 3, 1, 0])])
def test_shard_slices_tile_the_images(num_images, mb, world, want_counts):
    """Disjoint, covering, by the rule; the last global minibatch of each case is short, so some rank's slice of it is cut
    (30 images: rank 1 keeps 14 of 16) or empty (100 images: rank 1's fourth slice; 7 images: rank 3 owns nothing at all)."""
    from inclusivegan_amd.metrics.frechet_inception_distance import shard_slices
    per_rank = [shard_slices(num_images, mb, r, world) for r in range(world)]
    batches = -(-num_images // (world * mb))
    owner = np.full(num_images, -1)
    for r, slices in enumerate(per_rank):
        assert len(slices) == batches                                    # every rank walks every global minibatch
        for g, (begin, end) in enumerate(slices):
            lo, hi = g * world * mb + r * mb, g * world * mb + (r + 1) * mb        # the rule, restated: rows [r mb, (r + 1) mb) of batch g ...
            assert (begin, end) == (min(lo, num_images), min(hi, num_images))      # ... cut at num_images
            assert np.all(owner[begin:end] == -1)                        # disjoint
            owner[begin:end] = r
    assert np.all(owner >= 0)                                            # cover
    counts = [sum(e - b for b, e in s) for s in per_rank]
    assert sum(counts) == num_images and counts == want_counts
    assert any(e - b < mb for s in per_rank for b, e in s)             # a cut or empty slice is part of every case
    if (num_images, mb, world) == (100, 16, 2):
        assert per_rank[0][3] == (96, 100) and per_rank[1][3] == (100, 100)
    if (num_images, mb, world) == (7, 3, 4):
        assert per_rank[3] == [(7, 7)]
    for bad in (dict(rank=world), dict(rank=-1), dict(minibatch_per_gpu=0)):
        with pytest.raises(ValueError):
            shard_slices(**dict(dict(num_images=num_images, minibatch_per_gpu=mb, rank=0, world=world), **bad))


def test_run_metrics_main_names_the_launcher(tmp_path, monkeypatch, capsys):
    from inclusivegan_amd import run_metrics
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        run_metrics.main(['--data-dir', str(tmp_path), '--dataset', 'reals', '--network', 'n.pkl', '--num-gpus', '2',
                          '--result-dir', str(tmp_path / 'results')])
    assert e.value.code == 1
    out = capsys.readouterr().out
    assert 'python -m torch.distributed.run --nproc-per-node 2 -m inclusivegan_amd.run_metrics' in out
    assert not (tmp_path / 'results').exists()                          # refused before a run directory is made
    import inspect
    assert list(inspect.signature(run_metrics.run).parameters)[-1] == 'process_group'
