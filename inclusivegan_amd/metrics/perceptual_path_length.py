"""Perceptual Path Length (reference: metrics/perceptual_path_length.py:19-114; Karras et al., "A Style-Based Generator
Architecture for Generative Adversarial Networks" / "Analyzing and Improving the Image Quality of StyleGAN").

    PPL = mean over path positions of  LPIPS(G(path(t)), G(path(t + epsilon))) / epsilon^2,   1st..99th percentile kept

with the path a slerp in Z or a lerp in W, sampled everywhere ('full') or at the ends ('end'), the image optionally cropped
to the face region.  Everything it needs besides G is the LPIPS VGG16, which this package runs on its own HIP path.

What runs where: mapping / synthesis and the VGG convolutions are the kernels of training; the two endpoints of every pair
come from `igan_ppl_endpoints` (fp64 inside: the metric divides the effect of an epsilon-sized step by epsilon^2), crop /
box-mean / range change from `igan_ppl_crop_prep` (one pass over G's output, written in the VGG layout), the distances of
adjacent images from the LPIPS pair-table kernel on ONE interleaved feature batch (csrc/ppl.hip, csrc/lpips_dist.hip).
"""
import numpy as np
import torch

from .. import dnnlib
from .. import hip_ops
from ..dnnlib import tflib
from ..dnnlib.tflib import tfutil
from . import lpips as lpips_mod
from . import metric_base


def normalize(v):
    """Normalize batch of vectors (:19-20)."""
    return v / torch.sqrt(torch.sum(torch.square(v), dim=-1, keepdim=True))


def slerp(a, b, t):
    """Spherical interpolation of a batch of vectors (:23-30), in the precision of its inputs.  The metric itself takes its
    endpoints from hip_ops.ppl_endpoints_raw (the same formula in fp64)."""
    a = normalize(a)
    b = normalize(b)
    d = torch.sum(a * b, dim=-1, keepdim=True)
    p = t * torch.acos(d)
    c = normalize(b - d * a)
    d = a * torch.cos(p) + c * torch.sin(p)
    return normalize(d)


def crop_geometry(H, W, crop):
    """-> (y0, y1, x0, x1, factor): the face-region window of an H x W image (:85-87; the whole image without `crop`) and the
    box-mean factor that brings it to 256 rows (:90, taken AFTER the crop; images of fewer than 512 rows are left alone)."""
    H, W = int(H), int(W)
    if crop:
        c = H // 8
        y0, y1, x0, x1 = c * 3, c * 7, c * 2, c * 6
    else:
        y0, y1, x0, x1 = 0, H, 0, W
    factor = (y1 - y0) // 256
    return y0, y1, x0, x1, max(factor, 1)


def _percentile(a, q, how):
    try:
        return np.percentile(a, q, method=how)
    except TypeError:                   # NumPy before 1.22 calls the keyword `interpolation`
        return np.percentile(a, q, interpolation=how)


def reject_outliers(distances):
    """The distances between the 1st percentile (rounded down to a sample) and the 99th (rounded up), both kept (:111-113)."""
    distances = np.asarray(distances)
    lo = _percentile(distances, 1, 'lower')
    hi = _percentile(distances, 99, 'higher')
    return np.extract(np.logical_and(lo <= distances, distances <= hi), distances)


def num_minibatches(num_samples, minibatch_size):
    """T = ceil(num_samples / minibatch_size): the minibatches of a run."""
    return len(range(0, int(num_samples), int(minibatch_size)))


def minibatches_of_rank(T, rank, world):
    """The minibatches g of 0 .. T - 1 that rank `rank` of `world` evaluates, in its own order: g = rank, rank + world, ...
    (minibatch g is that rank's (g div world)-th).  Every g has exactly one owner."""
    T, rank, world = int(T), int(rank), int(world)
    if T < 0 or world < 1 or not 0 <= rank < world:
        raise ValueError('minibatches_of_rank: need T >= 0 and 0 <= rank < world')
    return list(range(rank, T, world))


class PPL(metric_base.MetricBase):
    """Per minibatch of m = num_gpus * minibatch_per_gpu pairs, every random number comes from tfutil's random source, in
    this order (a RecordingRandom / RandomTape records and replays a run):
        1. normal  [2m, latent_size]   the latents; rows 2i and 2i + 1 are the ends of pair i                     (:60)
        2. uniform [m]                 t, in [0, 1) for 'full'; for 'end' the same draw with maxval 0: all zero    (:61)
        3. normal  [1, 1, h, w]        one fresh noise image per synthesis layer, in layer order, written into the
                                       clone's noise%d variables and shared by the whole minibatch               (:57,80)
    Labels come from `_get_random_labels(m, Gs)` (the data set's own stream), each repeated for both ends of its pair (:62).
    All pairs of a run are evaluated on the current device; in one process `num_gpus` only sizes the minibatch.

    The LPIPS network is built the way training_loop builds it (`lpips_func_name`, seed `lpips_seed` = np_seed + 3 of the
    default run configuration), or passed in as `lpips_net`.

    Under a process group (`run(..., process_group=)`, `distances(..., process_group=)`) a minibatch is `minibatch_per_gpu`
    pairs whatever `num_gpus` says, minibatch g of the T = ceil(num_samples / minibatch_per_gpu) goes to rank g mod world
    (`minibatches_of_rank`), and all draws of a rank come, in the order above, from a private device generator seeded
    SHARD_SEED + rank (frechet_inception_distance.SHARD_SEED); labels are drawn from a restarted label stream for world x
    minibatch_per_gpu pairs per round and sliced to the rank's rows, as `_fold_shard_fakes` deals them.  A rank's work is
    a function of (rank, world) and the arguments alone (`rank_distances`: one process can replay any rank).  The
    per-minibatch distance vectors are gathered to every rank and put back in order of g -- the mean of the kept distances
    depends on the order -- and `reject_outliers` and the mean run on that array on every rank.  Every rank builds the LPIPS
    network from `lpips_seed`, so all hold the same weights."""

    multi_rank = True

    def __init__(self, num_samples, epsilon, space, sampling, crop, minibatch_per_gpu, Gs_overrides, lpips_net=None,
                 lpips_func_name='inclusivegan_amd.metrics.lpips.vgg16_zhang_perceptual', lpips_seed=1003, **kwargs):
        assert space in ['z', 'w']
        assert sampling in ['full', 'end']
        super().__init__(**kwargs)
        self.num_samples = num_samples
        self.epsilon = epsilon
        self.space = space
        self.sampling = sampling
        self.crop = crop
        self.minibatch_per_gpu = minibatch_per_gpu
        self.Gs_overrides = Gs_overrides
        self.lpips_net = lpips_net
        self.lpips_func_name = lpips_func_name
        self.lpips_seed = lpips_seed
        self._lpips_built = {}

    def _lpips(self, resolution, device):
        """The network passed in (used as it is: its variables do not depend on the image size), or one built per
        (resolution, device) and kept, so that a second run on a G of another output size gets a network of its own."""
        if self.lpips_net is not None:
            return self.lpips_net
        key = (int(resolution), str(device))
        if key not in self._lpips_built:
            with tfutil.use_random(tfutil.default_random()):
                self._lpips_built[key] = tflib.Network('lpips', func_name=self.lpips_func_name, resolution=resolution, device=device, seed=self.lpips_seed)
        return self._lpips_built[key]

    def _setup(self, Gs, Gs_kwargs, num_gpus):
        """Everything the minibatches share: the clone of Gs, its noise variables, the crop geometry, the LPIPS network."""
        st = dnnlib.EasyDict()
        st.Gs_kwargs = dict(Gs_kwargs)
        st.Gs_kwargs.update(self.Gs_overrides)
        st.synthesis_kwargs = dict(st.Gs_kwargs)
        st.synthesis_kwargs['randomize_noise'] = False
        st.m = int(num_gpus * self.minibatch_per_gpu)
        st.rank, st.world = 0, 1                            # labels are drawn for world x m pairs and cut to the rank's rows
        with tfutil.use_random(tfutil.default_random()):     # building a Network draws shape-only noise on the meta device:
            st.Gs = Gs.clone()                              # not a draw of the run, so not recorded and not replayed
        st.mapping, st.synthesis = st.Gs.components.mapping, st.Gs.components.synthesis
        st.noise_vars = [var for name, var in st.synthesis.vars.items() if name.startswith('noise')]
        H, W = (int(v) for v in st.Gs.output_shape[2:])
        y0, y1, x0, x1, st.factor = crop_geometry(H, W, self.crop)
        st.window = (y0, y1, x0, x1)
        h, w = (y1 - y0) // st.factor, (x1 - x0) // st.factor
        if h < 16 or w < 16 or h % 16 or w % 16:
            raise ValueError('PPL: the LPIPS network pools four times: its input must be a multiple of 16 on both sides, got '
                             '%d x %d (a %d x %d image%s)' % (h, w, H, W, ', cropped' if self.crop else ''))
        st.lpips = self._lpips(h, Gs.device)
        return st

    def _draw(self, st):
        """The random numbers of one minibatch, in the documented order; the fresh noise goes into the clone's variables."""
        dev, m = st.Gs.device, st.m
        lat_t01 = tfutil.random_normal([2 * m] + st.Gs.input_shape[1:], dev)
        lerp_t = tfutil.random_uniform([m], dev, 0.0, 1.0 if self.sampling == 'full' else 0.0)
        for var, fresh in zip(st.noise_vars, tfutil.random_normal_many([v.shape for v in st.noise_vars], dev)):
            var.copy_(fresh)
        labels = self._get_random_labels(st.world * m, st.Gs)[st.rank * m:(st.rank + 1) * m].repeat_interleave(2, dim=0)
        return lat_t01, lerp_t, labels

    def _minibatch(self, st):
        """LPIPS / epsilon^2 of m fresh pairs -> device tensor [m]."""
        lat_t01, lerp_t, labels = self._draw(st)

        # Interpolate in W or Z.
        if self.space == 'w':
            dlat_t01 = st.mapping.get_output_for(lat_t01, labels, **st.Gs_kwargs).to(torch.float32)
            dlat_e01 = hip_ops.ppl_endpoints_raw(dlat_t01, lerp_t, self.epsilon, 0)
        else:
            lat_e01 = hip_ops.ppl_endpoints_raw(lat_t01, lerp_t, self.epsilon, 1)
            dlat_e01 = st.mapping.get_output_for(lat_e01, labels, **st.Gs_kwargs)

        # Synthesize images with the same noise inputs for the entire minibatch; crop, downsample, [0, 255].
        images = st.synthesis.get_output_for(dlat_e01, **st.synthesis_kwargs).to(torch.float32)
        images = hip_ops.ppl_crop_prep_raw(images, st.window, st.factor)

        # Evaluate perceptual distance of the adjacent images: one VGG pass over the 2m interleaved images.
        feats = lpips_mod.features_of(st.lpips, images)
        return lpips_mod.adjacent_pair_distances_of(st.lpips, feats) * (1 / self.epsilon ** 2)

    def rank_distances(self, Gs, Gs_kwargs, rank, world):
        """The distance vectors [minibatch_per_gpu] of the minibatches rank `rank` of `world` owns, in its order (class
        docstring) -> device tensor [len(minibatches_of_rank(T, rank, world)), minibatch_per_gpu]."""
        from .frechet_inception_distance import SHARD_SEED
        with torch.no_grad():
            st = self._setup(Gs, Gs_kwargs, 1)
            st.rank, st.world = int(rank), int(world)
            self._label_rng = None
            with tfutil.use_random(tfutil.SeededRandom(Gs.device, SHARD_SEED + int(rank))):
                mine = [self._minibatch(st) for _g in minibatches_of_rank(num_minibatches(self.num_samples, st.m), rank, world)]
        return torch.stack(mine) if mine else torch.empty([0, st.m], device=Gs.device, dtype=torch.float32)

    def distances(self, Gs, Gs_kwargs=dict(is_validation=True), num_gpus=1, process_group=None):
        """The unfiltered per-pair distances LPIPS / epsilon^2 of ceil(num_samples / m) minibatches -> float32 [.. * m].  Under
        a process group every rank evaluates its minibatches and returns all of them, in order of g."""
        if process_group is not None:
            dist = torch.distributed
            rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
            mine = self.rank_distances(Gs, Gs_kwargs, rank, world)
            T = num_minibatches(self.num_samples, self.minibatch_per_gpu)
            out = torch.empty([T, int(self.minibatch_per_gpu)], device=mine.device, dtype=mine.dtype)
            owners = [[(g, g + 1) for g in minibatches_of_rank(T, r, world)] for r in range(world)]
            return metric_base.gather_rows(out, owners, mine, process_group).reshape(-1).cpu().numpy()
        with torch.no_grad():
            st = self._setup(Gs, Gs_kwargs, num_gpus)
            all_distances = [self._minibatch(st) for _begin in range(0, self.num_samples, st.m)]
        return torch.cat(all_distances).cpu().numpy()

    def _evaluate(self, Gs, Gs_kwargs, num_gpus):
        all_distances = self.distances(Gs, Gs_kwargs=Gs_kwargs, num_gpus=num_gpus, process_group=self._process_group)
        self._report_result(np.mean(reject_outliers(all_distances)))
