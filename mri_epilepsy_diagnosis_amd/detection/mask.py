"""detection/model_utils.py:118-246 — FCDMaskGenerator on the device: patches of a volume -> patch classifier -> patch map
[4, R, Z] -> neighbour vote -> voxel mask -> IoU.  R = Y // h strips per slice; the planes are the reference's patch kinds
(0 side, 1 middle, 2 middle mirrored, 3 side mirrored, model_utils.py:163-180).

The reference's inference half does not run as written; three defects are replaced by their evident intent:
  * model_utils.py:130-134  `_infer_patch` calls a global `model` one patch at a time.  Here it is the instance's model, in
    batches of `batch_size` patches that are gathered on the device.
  * model_utils.py:190-193  `patch_map_tensor[change_to_pos] = 1` indexes axis 0 with the integers 0 and 1 and overwrites two
    whole planes.  Here the two conditions are boolean masks, every cell decided from the map as it came in.
  * model_utils.py:212-215  `final_mask[..., -j:-j-h:-1, i]` is empty for j = 0 and one row off elsewhere.  Here the painted voxels
    are exactly the source voxels of channel 0 of the patch.
"""
import torch

from .. import _lib, ops
from ..ops import _ptr, _stream
from .model import PatchModel
from .patches import KINDS, PatchPlan, min_max_normalize


def _require_u8(who, t, shape):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("%s runs only on ROCm device tensors (got %s); there is no CPU fallback"
                           % (who, t.device if torch.is_tensor(t) else type(t).__name__))
    if t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s: expected a uint8 tensor of shape %s, got %s %s" % (who, tuple(shape), t.dtype, tuple(t.shape)))
    return t.contiguous()


def patch_vote(patch_map):
    """The neighbour vote of model_utils.py:183-194 on a uint8 [4, R, S] device map: a cell whose four neighbours in the
    (strip, slice) plane are all positive becomes 1, one with none becomes 0 (cells outside the map count as 0), every other
    cell stays; all cells are decided from the incoming map.  Returns a new map."""
    if patch_map.dim() != 3 or patch_map.shape[0] != KINDS:
        raise RuntimeError("patch_vote: expected a [4, R, S] map, got shape %s" % (tuple(patch_map.shape),))
    patch_map = _require_u8("patch_vote", patch_map, patch_map.shape)
    out = torch.empty_like(patch_map)
    _lib.check(_lib.lib().mri3d_patch_vote_u8(_ptr(patch_map), patch_map.shape[1], patch_map.shape[2], _ptr(out), _stream()), "patch_vote")
    return out


def paint_patches(patch_map, base_starts, shape, h, w):
    """Patch map [4, R, Z] + the [Z, R] starts of the base strips -> uint8 (X, Y, Z) mask: every voxel takes the value of the patch
    whose channel-0 footprint covers it (the middle patch where a side and a middle patch overlap), 0 elsewhere."""
    x, y, z = (int(s) for s in shape)
    r = y // int(h)
    patch_map = _require_u8("paint_patches", patch_map, (KINDS, r, z))
    if base_starts.dtype != torch.int32 or not base_starts.is_cuda or tuple(base_starts.shape) != (z, r) or not base_starts.is_contiguous():
        raise RuntimeError("paint_patches: the starts must be a contiguous int32 [Z, R] = %s device tensor" % ((z, r),))
    out = torch.empty((x, y, z), dtype=torch.uint8, device=patch_map.device)
    _lib.check(_lib.lib().mri3d_paint_patches_u8(_ptr(patch_map), _ptr(base_starts), x, y, z, int(h), int(w), _ptr(out), _stream()),
               "paint_patches")
    return out


class FCDMaskGenerator:
    """model_or_weights: a PatchModel, a state_dict, or the path of a saved one.  gm: the (X, Y, Z) grey-matter template on the
    device (or a PatchPlan of it); the plan and the patch table are made once here."""

    def __init__(self, model_or_weights, gm, h=16, w=32, batch_size=512):
        self.plan = gm if isinstance(gm, PatchPlan) else PatchPlan(gm, h, w)
        self.h, self.w, self.batch_size = self.plan.h, self.plan.w, int(batch_size)
        if isinstance(model_or_weights, torch.nn.Module):
            self.model = model_or_weights
        else:
            state = model_or_weights if isinstance(model_or_weights, dict) else torch.load(model_or_weights, map_location="cpu",
                                                                                           weights_only=True)
            self.model = PatchModel()
            self.model.load_state_dict(state)
        self.model.to(self.plan.device).eval()

    def predict_labels(self, img):
        """uint8 [P]: the model's class of every patch of the base grid, in table order."""
        patches = self.plan.patches(img, channels_last=True)
        out = torch.empty(len(self.plan), dtype=torch.uint8, device=self.plan.device)
        with torch.no_grad():
            for i in range(0, len(self.plan), self.batch_size):
                logits = self.model(patches[i:i + self.batch_size])
                # (N, 2) logits are the NDHWC memory of a (1, 2, N, 1, 1) volume: the device arg-max serves them as they lie
                out[i:i + self.batch_size] = ops.argmax_mask(logits.contiguous().t()[None, :, :, None, None]).view(-1)
        return out

    def map_of_labels(self, labels):
        """Patch labels [P] in table order -> uint8 patch map [4, R, Z] (0 where a strip has no such patch)."""
        r, z = self.plan.strips, self.plan.shape[2]
        patch_map = torch.zeros(KINDS * r * z, dtype=torch.uint8, device=self.plan.device)
        patch_map[self.plan.cells] = labels.to(torch.uint8)
        return patch_map.view(KINDS, r, z)

    def predict_patch_map(self, img):
        return self.map_of_labels(self.predict_labels(img))

    def postprocess(self, patch_map):
        return patch_vote(patch_map)

    def masking(self, patch_map):
        return paint_patches(patch_map, self.plan.base_starts, self.plan.shape, self.h, self.w)

    def get_mask(self, img):
        return self.masking(self.postprocess(self.predict_patch_map(img)))

    def get_iou(self, pred_mask, true_mask):
        if pred_mask.shape != true_mask.shape:
            raise RuntimeError("get_iou: wrong shape of masks, %s vs %s" % (tuple(pred_mask.shape), tuple(true_mask.shape)))
        n_and, n_or = (int(v) for v in ops.mask_overlap_counts(pred_mask, true_mask)[3:].tolist())
        return n_and / n_or if n_or else float("nan")

    def lesion_report(self, pred_mask, true_mask, connectivity=26):
        """Lesion-wise scores of a predicted mask against `true_mask > 0` (segmentation.components.lesion_scores): lesions hit
        and missed, true and false clusters, their sizes; the voxel-wise counterpart is `get_iou`."""
        from ..segmentation.components import lesion_scores
        if pred_mask.shape != true_mask.shape:
            raise RuntimeError("lesion_report: wrong shape of masks, %s vs %s" % (tuple(pred_mask.shape), tuple(true_mask.shape)))
        return lesion_scores(pred_mask, (true_mask > 0).to(torch.uint8), connectivity)

    def clusters(self, pred_mask, top_k=None, connectivity=26):
        """The connected clusters of a predicted mask, largest first (then by id): a dict of device tensors "ids" (int64, 1-based,
        numbered by first voxel in C order), "sizes" (int64) and "boxes" (int64 [K, 6]: inclusive min and max per axis), the first
        `top_k` of them."""
        from ..segmentation.components import components
        c = components(pred_mask, connectivity)
        order = torch.sort(c.sizes, descending=True, stable=True).indices
        if top_k is not None:
            order = order[:int(top_k)]
        return {"ids": order + 1, "sizes": c.sizes[order], "boxes": c.boxes[order]}

    def inference_pipeline(self, volume, mask=None):
        """model_utils.py:234-246 without the NIfTI reading and writing: (predicted uint8 mask, IoU against `mask > 0` or None)."""
        pred = self.get_mask(min_max_normalize(volume.to(torch.float32)))
        if mask is None:
            return pred, None
        return pred, self.get_iou(pred, (mask > 0).to(torch.uint8))
