"""Distance maps and ball morphology of device masks (ops.edt_sq / edt_threshold / signed_sqdist, csrc/distance.hip).

Everything here is a use of one exact integer transform, the squared Euclidean distance to the nearest zero voxel: its square
root is scipy.ndimage.distance_transform_edt, a threshold of it is a dilation or an erosion by a ball, two of those an opening or
a closing.  Masks are uint8 / bool device tensors (h, w), (d, h, w) or batches (n, d, h, w); no distance crosses from one volume
of a batch to the next.  Volumes are 1 mm isotropic, as for the surface distances: a radius is in voxels.

    gt_tol = dilate(gt, 2.5)                      # a hit tolerance of 2.5 mm around a lesion
    brain = erode(brain_mask, 2)                  # before znorm / tissue.segment
    clean = opening(pred, 1)
    maps = signed_distance_maps(class_map, 2, (1,))            # per step, for losses.BoundaryLoss
"""
import math

import torch

from .. import ops
from .components import _as_mask, _keep_table


def _r2(radius):
    """floor(radius^2) for a radius >= 0 (the ball holds the offsets with i^2 + j^2 + k^2 <= radius^2)."""
    radius = float(radius)
    if not radius >= 0.0 or math.isinf(radius):
        raise ValueError("radius must be a finite number >= 0, got %r" % (radius,))
    return int(math.floor(radius * radius + 1e-9))


def distance_transform_edt(mask):
    """float32 distances in voxels to the nearest zero voxel: sqrt of the exact integers, which equals
    scipy.ndimage.distance_transform_edt rounded to float32.  A volume without a zero voxel gives sqrt(EDT_INF) = 32511.0 everywhere
    (scipy leaves that case undefined)."""
    return torch.sqrt(ops.edt_sq(_as_mask("distance_transform_edt", mask)).to(torch.float32))


def dilate(mask, radius, out=None):
    """binary_dilation by the ball of `radius` (fractional allowed): the voxels within `radius` of a non-zero voxel.  uint8 0/1."""
    return ops.edt_threshold(_as_mask("dilate", mask), _r2(radius), greater=False, value=0, out=out)


def erode(mask, radius, outside=0, out=None):
    """binary_erosion by the ball of `radius`: the voxels further than `radius` from every zero voxel.  outside = 0 (scipy's
    border_value = 0, the default): the outside of the volume is zero voxels; outside = 1: it is not there.  uint8 0/1."""
    return ops.edt_threshold(_as_mask("erode", mask), _r2(radius), greater=True, outside_zero=not outside, out=out)


def opening(mask, radius):
    """binary_opening by the ball: erosion, then dilation (scipy's border_value = 0)."""
    return dilate(erode(mask, radius), radius)


def closing(mask, radius):
    """binary_closing by the ball: dilation, then erosion (scipy's border_value = 0: what touches the border after the dilation is
    eroded from there too)."""
    return erode(dilate(mask, radius), radius)


def fill_holes(mask):
    """scipy.ndimage.binary_fill_holes of one (d, h, w) or (h, w) mask: the mask plus every background voxel that no 6-connected
    background path joins to the volume's border (a (1, h, w) volume is all border, as for scipy).  A composition of what
    exists: the background is labelled (ops.label_components), the bounding boxes (ops.component_stats) say which components
    touch the border, the others are kept out of the background.  The component count is read from the device once."""
    mask = _as_mask("fill_holes", mask)
    background = (mask == 0).view(torch.uint8)
    labels, count = ops.label_components(background, 6)
    k = int(count)
    if k == 0:
        return torch.ones_like(mask)
    box = ops.component_stats(labels, k)["stats"][:, 2:8]
    ext = [1] * (3 - mask.dim()) + list(mask.shape)
    touches = torch.zeros(k, dtype=torch.bool, device=mask.device)
    for axis in range(3 - mask.dim(), 3):             # an (h, w) map has no border along d
        touches |= (box[:, 2 * axis] == 0) | (box[:, 2 * axis + 1] == ext[axis] - 1)
    outside = ops.select_components(labels, _keep_table(touches))
    return (outside == 0).view(torch.uint8)


def signed_distance_maps(class_map, classes, ids):
    """The int32 signed squared-distance maps (n, K, d, h, w) of a uint8 class map for the boundary loss (ops.signed_sqdist): per
    step, on the device, with no host synchronisation, so inside a captured training step too."""
    return ops.signed_sqdist(class_map, classes, ids)
