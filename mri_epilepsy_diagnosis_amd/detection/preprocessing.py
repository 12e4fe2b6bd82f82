"""Tensor-in / tensor-out counterparts of the reference's get_registered_img_and_mask and get_registered_img
(detection/preprocessing_utils.py:11-73): the FLIRT registration to the template on the device, without the file names and
without FAST bias correction (a tissue-segmentation EM, out of scope: DESIGN §6)."""
from .. import registration


def get_registered_img_and_mask(volume, template, mask=None, **register_kw):
    """Register `volume` to `template` (two (d, h, w) device volumes) and resample it, and `mask` with it (nearest neighbour), onto
    the template's grid: (registered_volume, registered_mask_or_None, matrix).  The matrix maps a template voxel index to a voxel
    index of `volume`; the outputs are exactly `registration.apply(volume, matrix, template.shape, label=mask)`.  Keyword arguments
    go to `registration.register` (dof=12 and cost='corratio' by default, FLIRT's)."""
    result = registration.register(volume, template, **register_kw)
    shape = tuple(template.shape)
    if mask is None:
        return registration.apply(volume, result.matrix, shape), None, result.matrix
    image, label = registration.apply(volume, result.matrix, shape, label=mask)
    return image, label, result.matrix


def get_registered_img(volume, template, **register_kw):
    """`volume` registered to `template` and resampled onto its grid."""
    return get_registered_img_and_mask(volume, template, None, **register_kw)[0]
