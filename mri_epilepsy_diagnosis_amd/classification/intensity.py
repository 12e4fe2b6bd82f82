"""Per-volume intensity densities on the device — what `plot_histogram` of the reference computes before it draws
(classification/transfer/full_sample_classification.ipynb cell 9):

    values = tensor.numpy().ravel()
    kernel = scipy.stats.gaussian_kde(values)
    positions = np.linspace(values.min(), values.max(), num=100)
    histogram = kernel(positions)

run there over 140 volumes and stacked into `resulted_hist` (classification/weights/data_140.csv), to judge by eye whether
harmonisation brought the scanner sites together.  Here the moments and the density come from `ops.intensity_moments` /
`ops.gaussian_kde` (csrc/intensity.hip); one (B, 8) moments row crosses to the host to decide whether scipy would have answered.
Plotting stays with the caller.
"""
import numpy as np
import torch

from .. import ops


def _check_rows(moments):
    """ValueError where scipy.stats.gaussian_kde cannot answer, decided from the moments rows alone."""
    for b, (count, bad, _lo, _hi, _mean, var) in enumerate(np.asarray(moments)[:, :6]):
        where = "" if len(moments) == 1 else " (volume %d)" % b
        if bad > 0:
            raise ValueError("intensity_histogram: %d non-finite voxel%s among the %d counted%s" % (bad, "" if bad == 1 else "s", count, where))
        if count < 2:
            raise ValueError("intensity_histogram: a density needs at least 2 counted voxels, got %d%s" % (count, where))
        if not var > 0:
            raise ValueError("intensity_histogram: the counted voxels have no variance (all %d equal)%s" % (count, where))


def _densities(rows, num_positions, mask, bw_method):
    moments = ops.intensity_moments(rows, mask)
    _check_rows(moments.cpu().numpy())
    positions, density = ops.gaussian_kde(rows, num_positions=num_positions, bw_method=bw_method, mask=mask, moments=moments)
    return positions.cpu().numpy(), density.cpu().numpy()


def intensity_histogram(tensor, num_positions=100, mask=None, bw_method=None):
    """(positions, histogram) of one volume, two float64 numpy arrays of `num_positions`: scipy.stats.gaussian_kde over all voxels
    of `tensor` (those `mask` selects, when given) at np.linspace(min, max, num_positions).  `bw_method` as in scipy: None / 'scott'
    / 'silverman' / a number.  Raises ValueError where scipy has no answer: fewer than 2 voxels, no variance, a non-finite voxel."""
    if not torch.is_tensor(tensor) or not tensor.is_cuda:
        raise RuntimeError("intensity_histogram runs only on a ROCm device tensor (got %s); there is no CPU fallback"
                           % (tensor.device if torch.is_tensor(tensor) else type(tensor).__name__))
    rows = tensor.to(torch.float32).reshape(1, -1)
    if mask is not None:
        mask = torch.as_tensor(mask, device=rows.device).reshape(1, -1)
        mask = mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0
    positions, density = _densities(rows, num_positions, mask, bw_method)
    return positions[0], density[0]


def histogram_table(volumes, num_positions=100, masks=None, bw_method=None):
    """The notebook's `resulted_hist`: one density row per volume, (positions, histograms) as two (len(volumes), num_positions)
    float64 numpy arrays.  `volumes` is a sequence of device tensors or one (B, ...) tensor; volumes of one size go through the
    kernels as one batch, others one by one.  `masks`, when given, pairs with `volumes`."""
    volumes = list(volumes)
    if not volumes:
        raise ValueError("histogram_table: no volumes")
    masks = [None] * len(volumes) if masks is None else list(masks)
    if len(masks) != len(volumes):
        raise ValueError("histogram_table: %d masks for %d volumes" % (len(masks), len(volumes)))
    same = len({v.numel() for v in volumes}) == 1 and (all(k is None for k in masks) or all(k is not None for k in masks))
    if same and all(torch.is_tensor(v) and v.is_cuda for v in volumes):
        rows = torch.stack([v.to(torch.float32).reshape(-1) for v in volumes])
        mask = None
        if masks[0] is not None:
            mask = torch.stack([torch.as_tensor(k, device=rows.device).reshape(-1) != 0 for k in masks])
        return _densities(rows, num_positions, mask, bw_method)
    out = [intensity_histogram(v, num_positions, k, bw_method) for v, k in zip(volumes, masks)]
    return np.stack([p for p, _ in out]), np.stack([h for _, h in out])
