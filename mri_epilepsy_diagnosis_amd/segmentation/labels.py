"""Label maps on the device: raw label ids (FreeSurfer parcellation ids in the reference's data) -> a uint8 class map, through a
lookup table that `ops.remap_labels` applies in one pass (csrc/labels.hip).

    lm = LabelMap.from_ids([17, 53, 1006, 2006])        # id k-th in the list -> class k + 1, everything else -> 0
    inputs, classes = prepare_batch_index(batch, device, lm)     # classes: uint8 (N, 1, D, H, W)
    loss = ops.softmax_dice_index_loss(model(inputs), classes)   # UNet(out_classes=lm.classes)

`LabelMap.binary_fcd()` is the reference's own rule (prepare_batch, segmentation/routine.py:185-196): ids in LIST_FCD -> 1 for the
first sample of a batch only, ids >= 1000 -> 1, 1 -> 1, everything else -> 0.
"""
import numpy as np
import torch

from .. import ops

MAX_LUT = 65536


def _as_lut(lut):
    lut = np.asarray(lut)
    if lut.ndim != 1 or not 1 <= lut.size <= MAX_LUT:
        raise ValueError("a label table has 1..%d entries, got shape %s" % (MAX_LUT, lut.shape))
    if lut.min() < 0 or lut.max() > 255:
        raise ValueError("classes must fit uint8")
    return np.ascontiguousarray(lut.astype(np.uint8))


class LabelMap:
    """lut[id] for integer ids in [0, len(lut)), `above` for values >= len(lut), `other` for everything else (negative,
    fractional, NaN).  `first_lut`, if given, replaces `lut` for the first sample of a batch (the reference's LIST_FCD quirk).
    The tables go to a device once, on first use there."""

    def __init__(self, lut, above=0, other=0, first_lut=None):
        self.lut = _as_lut(lut)
        self.first_lut = None if first_lut is None else _as_lut(first_lut)
        if self.first_lut is not None and self.first_lut.size != self.lut.size:
            raise ValueError("the first sample's table must have the length of the other")
        self.above, self.other = int(above), int(other)
        if not (0 <= self.above <= 255 and 0 <= self.other <= 255):
            raise ValueError("above / other must fit uint8")
        self._device = {}

    @classmethod
    def binary_fcd(cls):
        from .routine import LIST_FCD      # (routine imports this module)
        lut = np.zeros(1000, np.uint8)
        lut[1] = 1
        first = lut.copy()
        first[LIST_FCD] = 1
        return cls(lut, above=1, other=0, first_lut=first)

    @classmethod
    def from_ids(cls, ids):
        """The k-th id -> class k + 1; every other value -> 0 (background)."""
        return cls.from_groups({k + 1: [i] for k, i in enumerate(ids)})

    @classmethod
    def from_groups(cls, groups):
        """{class: ids}: every id of a group -> its class; every other value -> 0 (background)."""
        pairs = [(int(i), int(c)) for c, ids in groups.items() for i in ids]
        if not pairs:
            raise ValueError("no ids given")
        ids = [i for i, _ in pairs]
        if len(set(ids)) != len(ids):
            raise ValueError("an id is listed twice")
        if min(ids) < 0 or max(ids) >= MAX_LUT:
            raise ValueError("ids must lie in [0, %d)" % MAX_LUT)
        if min(c for _, c in pairs) < 1 or max(c for _, c in pairs) > 255:
            raise ValueError("classes must lie in 1..255 (0 is the background)")
        lut = np.zeros(max(ids) + 1, np.uint8)
        for i, c in pairs:
            lut[i] = c
        return cls(lut, above=0, other=0)

    @property
    def classes(self):
        """Number of classes a model needs for this map: the largest class it can produce, plus one."""
        top = max(int(self.lut.max()), self.above, self.other)
        if self.first_lut is not None:
            top = max(top, int(self.first_lut.max()))
        return top + 1

    def tables(self, device):
        """(lut, first_lut or None) as uint8 tensors on `device`; copied there on the first call only."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("LabelMap runs only on a ROCm device (got %s); there is no CPU fallback" % device)
        key = torch.cuda.current_device() if device.index is None else device.index
        t = self._device.get(key)
        if t is None:
            dev = torch.device("cuda", key)
            t = (torch.from_numpy(self.lut).to(dev), None if self.first_lut is None else torch.from_numpy(self.first_lut).to(dev))
            self._device[key] = t
        return t

    def __call__(self, labels, out_dtype=torch.uint8, out=None):
        """The class map of `labels` (N, ...) as `out_dtype` (uint8 or float32); out=labels remaps in place."""
        lut, first = self.tables(labels.device)
        if first is None or labels.dim() == 0 or labels.shape[0] == 0:
            return ops.remap_labels(labels, lut, self.above, self.other, out_dtype, out)
        if not labels.is_contiguous():
            if out is not None:
                raise RuntimeError("LabelMap: in-place remapping needs contiguous labels")
            labels = labels.contiguous()
        if out is None:
            out = torch.empty(labels.shape, dtype=out_dtype, device=labels.device)
        ops.remap_labels(labels[0], first, self.above, self.other, out=out[0])
        if labels.shape[0] > 1:
            ops.remap_labels(labels[1:], lut, self.above, self.other, out=out[1:])
        return out


def prepare_batch_index(batch, device, label_map):
    """`prepare_batch` for class-index training: the volume on the device and the label map as a uint8 (N, 1, D, H, W) class map.
    The raw labels (uint8 / int16 / int32 / float32) cross to the device as they are and are remapped there; the batch's own
    tensor is left alone."""
    from .routine import DATA, LABEL, MRI
    inputs = batch[MRI][DATA].to(device)
    labels = batch[LABEL][DATA].to(device)
    if labels.dim() == inputs.dim() - 1:
        labels = labels.unsqueeze(1)
    return inputs, label_map(labels, torch.uint8)
