"""Differentiable augmentation of everything D sees, reals and fakes, with gradients flowing back into G (Zhao et al.,
"Differentiable Augmentation for Data-Efficient GAN Training", NeurIPS 2020).  The reference has no such step; the loss functions
take it as `augment='color,translation,cutout'` (training/loss.py) and `run_training.py --diffaugment` switches it on.

The transform.  x is fp32 [n, C, H, W]; every sample gets one row of u [n, 8], fp32 uniforms in [0, 1) (column 7 is padding).
The policy is a bit set, 1 = color, 2 = translation, 4 = cutout, always applied in that order.  Integer parameters are

    draw(u, k) = min(floor(fl32(u * k)), k - 1)        fl32: the product rounded to fp32, np.float32(u) * np.float32(k);
                                                       the clamp holds the result below k whatever the rounding of the product does
  color        b = u0 - 1/2, s = 2 u1, c = u2 + 1/2;  m = mean of the sample's C H W inputs (fp64 sum, rounded to fp32 once);
               M = m + b;  per pixel p = mean over channels of x + b;   v_c = ((x_c + b - p) s + p - M) c + M
               (brightness, then saturation, then contrast: saturation keeps every pixel's channel mean, so the contrast mean is M)
  translation  S_y = floor(H / 8 + 1/2), t_y = draw(u4, 2 S_y + 1) - S_y; t_x likewise from u3 and W;
               w(i, j) = v(i + t_y, j + t_x) where that lies inside the image, else exactly 0
  cutout       K_y = floor(H / 2 + 1/2), r_y = 1 - K_y mod 2, o_y = draw(u6, H + r_y); rows o_y - K_y // 2 <= i < o_y - K_y // 2 + K_y
               are cut; columns likewise from u5 and W; a pixel whose row and column are both cut is exactly 0.

`diffaugment_torch` states this with torch operations (CPU tensors, and the yardstick of tools/augment_bench.py);
`hip_ops.diffaugment` is the fused HIP kernel every ROCm tensor goes through.
"""
import numpy as np
import torch

from ..dnnlib.tflib import tfutil
from .. import hip_ops

POLICIES = ('color', 'translation', 'cutout')      # bit k of the policy set is POLICIES[k]
COLOR, TRANSLATION, CUTOUT = 1, 2, 4

#----------------------------------------------------------------------------

def parse_policy(policy):
    """'color,translation,cutout' -> 7.  None and '' give 0; an unknown name raises ValueError."""
    if policy is None or policy == '':
        return 0
    if not isinstance(policy, str):
        raise ValueError('augmentation policy must be a comma-separated string of %s (got %r)' % (', '.join(POLICIES), policy))
    bits = 0
    for name in policy.split(','):
        if name.strip() not in POLICIES:
            raise ValueError('unknown augmentation %r; known: %s' % (name, ', '.join(POLICIES)))
        bits |= 1 << POLICIES.index(name.strip())
    return bits

def policy_names(bits):
    """7 -> ['color', 'translation', 'cutout'] (the order of application)."""
    if bits < 0 or bits >> len(POLICIES):
        raise ValueError('unknown augmentation policy bits %d' % bits)
    return [name for k, name in enumerate(POLICIES) if bits >> k & 1]

#----------------------------------------------------------------------------

def _draw_np(u, k):
    return np.minimum(np.floor(u.astype(np.float32) * np.float32(k)).astype(np.int64), k - 1)

def parameters(u, H, W):
    """Host statement of the parameters the rows of u [n, 8] select for H x W images: a dict of arrays of length n.
    brightness, saturation, contrast: fp32.  t_y, t_x: the translation.  cut_y0, cut_y1, cut_x0, cut_x1: the cut rows / columns
    as half-open ranges intersected with the image.  shift_y, shift_x, cut_h, cut_w: the sizes S and K (the same for every row)."""
    u = np.asarray(u, dtype=np.float32).reshape(-1, 8)
    n = u.shape[0]
    Sy, Sx = int(np.floor(H / 8 + 0.5)), int(np.floor(W / 8 + 0.5))
    Ky, Kx = int(np.floor(H / 2 + 0.5)), int(np.floor(W / 2 + 0.5))
    oy = _draw_np(u[:, 6], H + 1 - Ky % 2) - Ky // 2
    ox = _draw_np(u[:, 5], W + 1 - Kx % 2) - Kx // 2
    full = lambda v: np.full(n, v, dtype=np.int64)
    return dict(
        brightness=u[:, 0] - np.float32(0.5), saturation=np.float32(2) * u[:, 1], contrast=u[:, 2] + np.float32(0.5),
        t_y=_draw_np(u[:, 4], 2 * Sy + 1) - Sy, t_x=_draw_np(u[:, 3], 2 * Sx + 1) - Sx,
        cut_y0=np.clip(oy, 0, H), cut_y1=np.clip(oy + Ky, 0, H), cut_x0=np.clip(ox, 0, W), cut_x1=np.clip(ox + Kx, 0, W),
        shift_y=full(Sy), shift_x=full(Sx), cut_h=full(Ky), cut_w=full(Kx))

#----------------------------------------------------------------------------

def _draw(u, k):
    return torch.clamp(torch.floor(u.float() * float(k)), max=k - 1).long()      # on u's device: no host synchronisation

def diffaugment_torch(x, u, bits):
    """The transform with torch operations, differentiable by autograd, on whatever device x lives.  The arithmetic runs in x's
    dtype (fp32 in training; fp64 states the real-arithmetic transform for tests); the integer parameters always come from the
    fp32 product."""
    if bits < 0 or bits >> len(POLICIES):
        raise ValueError('unknown augmentation policy bits %d' % bits)
    n, C, H, W = (int(v) for v in x.shape)
    if tuple(u.shape) != (n, 8):
        raise ValueError('diffaugment: u must be [%d, 8] (got %s)' % (n, tuple(u.shape)))
    uf = u.to(x.dtype)
    if bits & COLOR:
        b = (uf[:, 0] - 0.5).view(n, 1, 1, 1)
        s = (2.0 * uf[:, 1]).view(n, 1, 1, 1)
        c = (uf[:, 2] + 0.5).view(n, 1, 1, 1)
        m = (x.double().sum(dim=(1, 2, 3), keepdim=True) / float(C * H * W)).to(x.dtype)
        M = m + b
        xb = x + b
        p = xb.mean(dim=1, keepdim=True)
        x = ((xb - p) * s + p - M) * c + M
    ii = torch.arange(H, device=x.device).view(1, H)
    jj = torch.arange(W, device=x.device).view(1, W)
    if bits & TRANSLATION:
        Sy, Sx = (H + 4) // 8, (W + 4) // 8
        si = ii + (_draw(u[:, 4], 2 * Sy + 1) - Sy).view(n, 1)
        sj = jj + (_draw(u[:, 3], 2 * Sx + 1) - Sx).view(n, 1)
        inside = ((si >= 0) & (si < H)).view(n, 1, H, 1) & ((sj >= 0) & (sj < W)).view(n, 1, 1, W)
        idx = (si.clamp(0, H - 1) * W).view(n, H, 1) + sj.clamp(0, W - 1).view(n, 1, W)
        x = x.reshape(n, C, H * W).gather(2, idx.view(n, 1, H * W).expand(n, C, H * W)).view(n, C, H, W)
        x = torch.where(inside, x, torch.zeros((), dtype=x.dtype, device=x.device))
    if bits & CUTOUT:
        Ky, Kx = (H + 1) // 2, (W + 1) // 2
        y0 = (_draw(u[:, 6], H + 1 - Ky % 2) - Ky // 2).view(n, 1)
        x0 = (_draw(u[:, 5], W + 1 - Kx % 2) - Kx // 2).view(n, 1)
        cut = ((ii >= y0) & (ii < y0 + Ky)).view(n, 1, H, 1) & ((jj >= x0) & (jj < x0 + Kx)).view(n, 1, 1, W)
        x = torch.where(cut, torch.zeros((), dtype=x.dtype, device=x.device), x)
    return x

#----------------------------------------------------------------------------

def augment(x, u, bits):
    """T_u(x): ROCm tensors through the fused HIP kernel (hip_ops.diffaugment), CPU tensors through the torch statement."""
    if x.is_cuda:
        return hip_ops.diffaugment(x, u, bits)
    return diffaugment_torch(x, u, bits)

def DiffAugment(x, bits):
    """Augment the batch x under the policy bits with ONE draw tfutil.random_uniform([n, 8]).  bits == 0 returns x itself and draws nothing."""
    if not bits:
        return x
    return augment(x, tfutil.random_uniform([int(x.shape[0]), 8], x.device), bits)
