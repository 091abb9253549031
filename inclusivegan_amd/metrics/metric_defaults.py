"""Default metric definitions (reference: metrics/metric_defaults.py:13-29): every entry of the reference's table, prd30k
for the reference's stand-alone precision-recall-distributions script, and two metrics the reference never had: dc50k5 --
density and coverage (Naeem et al., ICML 2020), per-real coverage with k = 5 -- and kid50k -- the Kernel Inception Distance
(Binkowski et al., ICLR 2018), the unbiased MMD^2 estimator with the cubic polynomial kernel over 100 subsets of at most 1000
rows.  fid30k, pr50k3, dc50k5, kid50k, prd30k, is50k and ls take the network whose pickle is not available as an injected callable (`feature_fn`, `classify_fn`,
`classify_fns`: pass it through the metric's keyword arguments).  The five ppl* entries need no injected network: besides G
they use the LPIPS VGG16 this package runs for the reconstruction loss.  Under a process group (MetricGroup.run(..., process_group=)) every
entry but `ls` is evaluated by all ranks (`multi_rank`); `ls` runs on rank 0 alone."""
from ..dnnlib import EasyDict

metric_defaults = EasyDict([(args.name, args) for args in [
    EasyDict(name='mode_counts_24k', func_name='metrics.mode_counts.mode_counts', num_images=24000, minibatch_per_gpu=32),
    EasyDict(name='KL24k', func_name='metrics.KL.KL', num_images=24000, minibatch_per_gpu=32),
    EasyDict(name='fid30k', func_name='metrics.frechet_inception_distance.FID', num_images=30000, minibatch_per_gpu=8),
    EasyDict(name='is50k', func_name='metrics.inception_score.IS', num_images=50000, num_splits=10, minibatch_per_gpu=8),
    EasyDict(name='ppl_zfull', func_name='metrics.perceptual_path_length.PPL', num_samples=50000, epsilon=1e-4, space='z', sampling='full', crop=True, minibatch_per_gpu=4, Gs_overrides=dict(dtype='float32', mapping_dtype='float32')),
    EasyDict(name='ppl_wfull', func_name='metrics.perceptual_path_length.PPL', num_samples=50000, epsilon=1e-4, space='w', sampling='full', crop=True, minibatch_per_gpu=4, Gs_overrides=dict(dtype='float32', mapping_dtype='float32')),
    EasyDict(name='ppl_zend', func_name='metrics.perceptual_path_length.PPL', num_samples=50000, epsilon=1e-4, space='z', sampling='end', crop=True, minibatch_per_gpu=4, Gs_overrides=dict(dtype='float32', mapping_dtype='float32')),
    EasyDict(name='ppl_wend', func_name='metrics.perceptual_path_length.PPL', num_samples=50000, epsilon=1e-4, space='w', sampling='end', crop=True, minibatch_per_gpu=4, Gs_overrides=dict(dtype='float32', mapping_dtype='float32')),
    EasyDict(name='ppl2_wend', func_name='metrics.perceptual_path_length.PPL', num_samples=50000, epsilon=1e-4, space='w', sampling='end', crop=False, minibatch_per_gpu=4, Gs_overrides=dict(dtype='float32', mapping_dtype='float32')),
    EasyDict(name='pr50k3', func_name='metrics.precision_recall.PR', num_images=50000, nhood_size=3, minibatch_per_gpu=8, row_batch_size=10000, col_batch_size=10000),
    EasyDict(name='dc50k5', func_name='metrics.density_coverage.DC', num_images=50000, nhood_size=5, minibatch_per_gpu=8, row_batch_size=10000, col_batch_size=10000),
    EasyDict(name='kid50k', func_name='metrics.kernel_inception_distance.KID', num_images=50000, num_subsets=100, max_subset_size=1000, minibatch_per_gpu=8),
    EasyDict(name='prd30k', func_name='metrics.prd_score.PRD', num_images=30000, num_clusters=20, num_angles=1001, num_runs=10, minibatch_per_gpu=8),
    EasyDict(name='ls', func_name='metrics.linear_separability.LS', num_samples=200000, num_keep=100000, attrib_indices=range(40), minibatch_per_gpu=4),
]])
