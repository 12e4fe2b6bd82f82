"""Training losses against a uint8 class map, as callables `loss(logits, class_map)` for `routine.run_epoch`:

    lm = LabelMap.binary_fcd()
    prepare = lambda batch, device: prepare_batch_index(batch, device, lm)
    w = class_weights(class_map, lm.classes, "inverse_sqrt")            # from exact device counts, once, before training
    run_epoch(epoch, Action.TRAIN, loader, model, optimizer, loss_fn=DiceCELoss(weight=w), prepare=prepare)

All three run csrc/ce_loss.hip (ops.softmax_ce_index_loss / ops.softmax_dice_ce_index_loss): one pass over the logits forward, one
backward, whatever the combination.  The class weights are host numbers held by the loss; they go to a device once, the first
time that device is seen, in a table shared by every loss with the same weights — never inside a captured training step.  Two
losses built with equal settings are equal and hash alike, so `parallel.StepCache` replays the step it captured for the first.

BoundaryLoss and DiceBoundaryLoss (csrc/distance.hip) add the boundary term of Kervadec et al.: the signed distance maps of the
class map are computed on the device inside every step.
"""
import numpy as np
import torch

from .. import ops

RULES = ("inverse", "inverse_sqrt", "median")

# (weights as float32 bytes, device index) -> the device tensor; kept for the life of the process: a captured step reads it
_device_weights = {}


def _host_weights(weight):
    """None, or the weights as a tuple of float32 values (a device tensor is read back once, here)."""
    if weight is None:
        return None
    w = weight.detach().cpu().numpy() if torch.is_tensor(weight) else np.asarray(weight)
    w = np.ascontiguousarray(w, dtype=np.float32)
    if w.ndim != 1 or not 2 <= w.size <= 32 or not np.all(np.isfinite(w)) or w.min() < 0:
        raise ValueError("class weights are 2..32 finite numbers >= 0, got %r" % (weight,))
    return tuple(float(v) for v in w)


class _IndexLoss:
    """Settings -> a callable; equality and hash go by the settings."""

    def __init__(self, dice_weight, ce_weight, weight, gamma):
        self.dice_weight, self.ce_weight, self.gamma = float(dice_weight), float(ce_weight), float(gamma)
        self.weight = _host_weights(weight)
        ops._ce_settings(type(self).__name__, self.gamma, self.dice_weight, self.ce_weight)
        if torch.is_tensor(weight) and weight.is_cuda:
            self._weight_on(weight.device)                # known device: the table is there before the first step

    def _key(self):
        return (self.dice_weight, self.ce_weight, self.gamma, self.weight)

    def __eq__(self, other):
        return isinstance(other, _IndexLoss) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "%s(dice_weight=%g, ce_weight=%g, gamma=%g, weight=%s)" % ((type(self).__name__,) + self._key())

    def _weight_on(self, device):
        if self.weight is None:
            return None
        if device.type != "cuda":
            raise RuntimeError("%s runs only on a ROCm device (got %s); there is no CPU fallback" % (type(self).__name__, device))
        key = (self.weight, torch.cuda.current_device() if device.index is None else device.index)
        t = _device_weights.get(key)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("%s: the class weights must reach the device before a step is captured" % type(self).__name__)
            t = torch.tensor(self.weight, dtype=torch.float32).to(torch.device("cuda", key[1]))
            _device_weights[key] = t
        return t

    def __call__(self, logits, class_map):
        w = self._weight_on(logits.device)
        # (dice_weight == 0 selects the CE-only kernels inside)
        return ops.softmax_dice_ce_index_loss(logits, class_map, self.dice_weight, self.ce_weight, w, self.gamma)


class CrossEntropyLoss(_IndexLoss):
    """Voxel-wise cross-entropy (F.cross_entropy with class weights and ignored voxels, mean reduction); gamma > 0: focal."""

    def __init__(self, weight=None, gamma=0.0):
        super().__init__(0.0, 1.0, weight, gamma)


class FocalLoss(_IndexLoss):
    """Focal loss: the voxel's cross-entropy times (1 - p_y)^gamma, gamma in [1, 8]."""

    def __init__(self, gamma=2.0, weight=None):
        super().__init__(0.0, 1.0, weight, gamma)


class DiceCELoss(_IndexLoss):
    """dice_weight * softmax-Dice + ce_weight * cross-entropy (focal with gamma > 0), fused: the logits are read once per pass."""

    def __init__(self, dice_weight=1.0, ce_weight=1.0, weight=None, gamma=0.0):
        super().__init__(dice_weight, ce_weight, weight, gamma)


class _BoundaryLoss:
    """dice_weight * index Dice + boundary_weight * boundary term; equality and hash go by the settings."""

    def __init__(self, dice_weight, boundary_weight, ids, classes):
        self.dice_weight, self.boundary_weight = float(dice_weight), float(boundary_weight)
        self.classes, self.ids = ops._class_ids(type(self).__name__, classes, ids)
        if not (0.0 <= self.dice_weight < float("inf") and 0.0 < self.boundary_weight < float("inf")):
            raise ValueError("%s: dice_weight must be finite and >= 0, boundary_weight finite and > 0, got %r and %r"
                             % (type(self).__name__, dice_weight, boundary_weight))

    def _key(self):
        return (self.dice_weight, self.boundary_weight, self.ids, self.classes)

    def __eq__(self, other):
        return isinstance(other, _BoundaryLoss) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "%s(dice_weight=%g, boundary_weight=%g, ids=%s, classes=%d)" % ((type(self).__name__,) + self._key())

    def __call__(self, logits, class_map):
        if logits.shape[1] != self.classes:
            raise RuntimeError("%s: built for %d classes, the logits have %d" % (type(self).__name__, self.classes, logits.shape[1]))
        maps = ops.signed_sqdist(class_map, self.classes, self.ids)       # per step: the targets change with the augmentation
        loss = self.boundary_weight * ops.softmax_boundary_loss(logits, maps, self.ids)
        if self.dice_weight > 0.0:
            loss = loss + self.dice_weight * ops.softmax_dice_index_loss(logits, class_map)
        return loss


class BoundaryLoss(_BoundaryLoss):
    """Boundary loss of Kervadec et al. (MIDL 2019) for the classes `ids` of a `classes`-class map: the mean of softmax(logits)[id]
    times the signed distance to the class's boundary (negative inside), whose gradient does not vanish when prediction and lesion
    do not overlap.  The signed maps are made on the device inside the step (csrc/distance.hip), with no host synchronisation."""

    def __init__(self, ids=(1,), classes=2):
        super().__init__(0.0, 1.0, ids, classes)


class DiceBoundaryLoss(_BoundaryLoss):
    """dice_weight * softmax-Dice (ops.softmax_dice_index_loss) + boundary_weight * BoundaryLoss, two operators on the same logits.
    Two losses with equal settings are equal and hash alike, so `parallel.StepCache` replays the step it captured for the first;
    the weights are part of the settings, so a re-weighted schedule (the paper's rebalancing of the two terms over the epochs)
    costs one new capture per distinct (dice_weight, boundary_weight) pair: step the weights a few times a run, not every epoch."""

    def __init__(self, dice_weight=1.0, boundary_weight=1.0, ids=(1,), classes=2):
        super().__init__(dice_weight, boundary_weight, ids, classes)


def weights_from_counts(counts, rule):
    """Class weights from a histogram (host numbers): "inverse" 1 / count, "inverse_sqrt" 1 / sqrt(count), "median"
    median(count over the classes present) / count; normalised to mean 1 over the classes present, 0 for a class that does not
    occur.  float32 numpy array."""
    if rule not in RULES:
        raise ValueError("rule must be one of %s, got %r" % (RULES, rule))
    n = np.asarray(counts, dtype=np.float64)
    if n.ndim != 1 or n.size < 2 or n.min() < 0:
        raise ValueError("counts are a 1-D histogram of at least 2 classes, got %r" % (counts,))
    present = n > 0
    w = np.zeros_like(n)
    if present.any():
        c = n[present]
        w[present] = {"inverse": 1.0 / c, "inverse_sqrt": 1.0 / np.sqrt(c), "median": np.median(c) / c}[rule]
        w[present] /= w[present].mean()
    return w.astype(np.float32)


def class_weights(class_map, classes, rule="inverse"):
    """Class weights of a uint8 device class map (any shape; labels >= classes are ignored) by `rule` (see weights_from_counts),
    from exact device counts — the diagonal of ops.confusion_counts(y, y, C) — as a float32 tensor of `classes` entries on the
    map's device.  Call it outside the training step: the counts come to the host once."""
    conf, _ = ops.confusion_counts(class_map, class_map, classes)
    w = weights_from_counts(torch.diagonal(conf).cpu().numpy(), rule)
    return torch.from_numpy(w).to(class_map.device)
