"""Tensor-in / tensor-out counterparts of the reference's get_registered_img_and_mask and get_registered_img
(detection/preprocessing_utils.py:11-73): the FLIRT registration to the template on the device, without the file names, and
FAST's bias-corrected image from the tissue-class estimator of `tissue` (its model, not a clone of FAST: DESIGN §4.17)."""
from .. import registration, tissue


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


def get_registered_img_bias_and_mask(volume, template, mask=None, tissue_kw=None, **register_kw):
    """The reference's triple plus the matrix: (registered, restored, registered_mask_or_None, matrix).  `registered`, the mask
    and the matrix are `get_registered_img_and_mask`'s; `restored` is the registered image with its bias field removed
    (`tissue.bias_correct`, estimated over the registered mask when there is one).  `tissue_kw` goes to `tissue.segment`
    (classes, order, iterations, or a `mask` of the template's shape that replaces the registered one)."""
    image, label, matrix = get_registered_img_and_mask(volume, template, mask, **register_kw)
    kw = dict(tissue_kw or {})
    kw.setdefault("mask", label)
    return image, tissue.bias_correct(image, **kw), label, matrix
