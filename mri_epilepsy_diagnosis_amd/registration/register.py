"""Affine registration of a subject's volume to a template on the device: the image pyramid, the batched cost evaluation on
csrc/register.hip's joint-histogram kernel, and the coarse-to-fine driver.  The device counterpart of the FLIRT call in the
reference's detection/preprocessing_utils.py:11-73 (correlation ratio, 12 degrees of freedom, trilinear resampling)."""
import collections

import numpy as np
import torch

from .. import ops
from ..classification.preprocessing import percentile
from . import affine as _affine

MAX_CANDIDATES = 64     # per joint_histogram launch
RANGE_PERCENTILES = (1.0, 99.0)

Registration = collections.namedtuple("Registration", ["matrix", "cost", "overlap", "trace"])


def _device_volume(who, what, t):
    if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 3:
        raise RuntimeError("%s: %s must be a (d, h, w) ROCm device tensor (got %s); there is no CPU fallback"
                           % (who, what, getattr(t, "device", type(t))))
    return t.to(torch.float32).contiguous()


class Pyramid:
    """`levels` volumes, level l + 1 the 2x mean of level l (`ops.downsample2`), and per level the quantisation range
    (lo, hi) = the 1st and 99th percentile of the level's voxels (`preprocessing.percentile`).  `matrix_at` conjugates a level-0
    matrix to a level (`affine.level_matrix`)."""

    def __init__(self, volume, levels):
        if int(levels) < 1:
            raise ValueError("Pyramid: levels must be >= 1, got %r" % (levels,))
        self.volumes = [_device_volume("Pyramid", "volume", volume)]
        for _ in range(int(levels) - 1):
            if min(self.volumes[-1].shape) < 2:
                break
            self.volumes.append(ops.downsample2(self.volumes[-1]))
        self.ranges = []
        for v in self.volumes:
            lo, hi = (float(q) for q in percentile(v.reshape(-1), RANGE_PERCENTILES))
            self.ranges.append((lo, hi if hi > lo else lo + 1.0))

    def __len__(self):
        return len(self.volumes)

    def scale(self, level, bins):
        """(lo, scale) that spread the level's range over `bins` bins."""
        lo, hi = self.ranges[level]
        return lo, bins / (hi - lo)

    @staticmethod
    def matrix_at(matrix, level):
        return _affine.level_matrix(matrix, level)


def _mask_pyramid(mask, levels):
    out = [mask.to(torch.float32).contiguous()]
    for _ in range(levels - 1):
        out.append(ops.downsample2(out[-1]))
    return [m >= 0.5 for m in out]


def _dof_schedule(levels, dof):
    """Degrees of freedom per level, level 0 first: the requested dof at full resolution, at most 9 one level up, at most 6 above."""
    return [dof if l == 0 else min(dof, 9) if l == 1 else min(dof, 6) for l in range(levels)]


def register(moving, fixed, fixed_mask=None, dof=12, cost="corratio", bins=64, levels=4, search_angles=None,
             fixed_spacing=(1, 1, 1), moving_spacing=(1, 1, 1), step=2.0, tol=0.05, min_count=None, max_iter=200):
    """Register `moving` to `fixed` (two (d, h, w) device volumes): returns Registration(matrix, cost, overlap, trace).
        matrix   (3, 4) float64, fixed voxel index -> moving voxel index (what `apply` and `ops.resample_affine` take)
        cost     the final cost at full resolution; overlap: the samples it counted
        trace    one dict per level, coarsest first: level, dof, cost, overlap, iterations, calls, evaluations, params
    fixed_mask (bool / uint8, fixed's shape) limits the fixed voxels that count.  dof 3, 6, 9 or 12; cost 'corratio', 'mi' or
    'nmi'.  search_angles: angles in radians tried on every axis at the coarsest level (all combinations, in launches of at most
    64 candidates) before the search starts.  step, tol: the first translation step and the stopping step at full resolution, in
    voxels of level 0 times 2^level at the coarser levels.  min_count: samples below which a candidate costs +inf, by default a
    quarter of the level's counted fixed voxels; a given value is meant for level 0 and divided by 8 per level above it."""
    if dof not in _affine.DOF_CHOICES:
        raise ValueError("register: dof must be one of %s, got %r" % (_affine.DOF_CHOICES, dof))
    if cost not in ops.HIST_COST_KINDS:
        raise ValueError("register: cost must be one of %s, got %r" % (sorted(ops.HIST_COST_KINDS), cost))
    fixed = _device_volume("register", "fixed", fixed)
    moving = _device_volume("register", "moving", moving)
    if fixed_mask is not None and (not torch.is_tensor(fixed_mask) or tuple(fixed_mask.shape) != tuple(fixed.shape) or not fixed_mask.is_cuda):
        raise RuntimeError("register: fixed_mask must be a device tensor of the fixed volume's shape %s" % (tuple(fixed.shape),))
    pf, pm = Pyramid(fixed, levels), Pyramid(moving, levels)
    nlev = min(len(pf), len(pm))
    masks = _mask_pyramid(fixed_mask, nlev) if fixed_mask is not None else [None] * nlev
    fshape, mshape = tuple(fixed.shape), tuple(moving.shape)

    def to_matrix(p):
        return _affine.params_to_matrix(p, fshape, mshape, fixed_spacing, moving_spacing)

    x = np.zeros(12)
    trace = []
    final = None
    for level, level_dof in reversed(list(enumerate(_dof_schedule(nlev, dof)))):
        f_lo, f_scale = pf.scale(level, bins)
        m_lo, m_scale = pm.scale(level, bins)
        fixed_bins = ops.quantize_bins(pf.volumes[level], f_lo, f_scale, bins, mask=masks[level])
        counted = int((fixed_bins != 255).sum())
        need = float(min_count) / 8 ** level if min_count is not None else counted / 4.0
        last = {}

        def evaluate(matrices, level=level, fixed_bins=fixed_bins, m_lo=m_lo, m_scale=m_scale, need=need, last=last):
            out = []
            for i in range(0, len(matrices), MAX_CANDIDATES):
                chunk = np.stack([_affine.level_matrix(m, level) for m in matrices[i:i + MAX_CANDIDATES]])
                hist = ops.joint_histogram(fixed_bins, pm.volumes[level], torch.from_numpy(chunk), m_lo, m_scale, bins)
                out.append(ops.histogram_costs(hist, cost, need).cpu().numpy())
            res = np.concatenate(out)
            last["n"] = res[:, 1]
            return res[:, 0]

        if search_angles is not None and level == nlev - 1:
            angles = [float(a) for a in search_angles]
            grid = [np.concatenate([x[:3], [a, b, c], x[6:]]) for a in angles for b in angles for c in angles]
            costs = evaluate([to_matrix(p) for p in grid])
            x = grid[int(np.argmin(costs))]
        x, fx, info = _affine.optimise(evaluate, x, level_dof, _affine.step_vector(step * 2 ** level, level_dof), tol * 2 ** level,
                                       to_matrix, max_iter=max_iter)
        fx = float(evaluate([to_matrix(x)])[0])
        final = (fx, float(last["n"][0]))
        trace.append(dict(level=level, dof=level_dof, cost=fx, overlap=final[1], params=x.copy(), **info))
    return Registration(to_matrix(x), final[0], final[1], trace)


def apply(moving, matrix, fixed_shape, label=None, pad=0.0):
    """Resample `moving` (trilinear) and, when given, `label` (nearest) onto a grid of `fixed_shape` under a registration's matrix:
    the volume, or (volume, label)."""
    image, lab = ops.resample_affine(_device_volume("apply", "moving", moving), label, matrix, fixed_shape, pad)
    return image if label is None else (image, lab)
