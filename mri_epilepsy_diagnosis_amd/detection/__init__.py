"""The patch-based FCD detector of the reference's detection/ on the device: mirrored patch pairs along the grey-matter
template (patches), the patch classifier (model), its training loop (routine) and the lesion mask (mask)."""
from .mask import FCDMaskGenerator  # noqa: F401
from .model import ConvolutionBlock, PatchModel  # noqa: F401
from .patches import (PatchPlan, get_all_patches_and_labels, get_image_patches, get_only_patches,  # noqa: F401
                      patch_table, strip_starts)
