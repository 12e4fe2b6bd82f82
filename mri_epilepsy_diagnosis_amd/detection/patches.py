"""Mirrored left/right patch pairs along the grey-matter template (reference detection/patch_utils.py) on the device.

Everything here is one closed form (csrc/detection.hip).  Slice z of a (X, Y, Z) array A is B = np.rot90(A[:, :, z]),
B[r, c] = A[c, Y-1-r, z]; a strip is the h rows r = row0 .. row0+h-1; a patch is the triple (z, row0, col0) with

    channel 0   B[row0+i, col0+t]        channel 1   B[row0+i, X-1-col0-t]        i < h, t < w

and the four patch kinds of the reference are col0 = start, X-start-w (sides, only where start < mid) and col0 = mid, X-mid-w
(middles), mid = X//2 - w, start the first column of the strip that holds a template value > 0 (patch_utils.py:30-70).
The template decides the patches, so it is planned once (`PatchPlan`) and every volume registered to it is one gather launch.
"""
import numpy as np
import torch

from .. import _lib
from ..ops import _ptr, _stream

KINDS = 4   # patch-map planes: 0 side, 1 middle, 2 middle mirrored, 3 side mirrored (model_utils.py:163-180)


def _require(who, t, dtype, shape=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("%s runs only on ROCm device tensors (got %s); there is no CPU fallback"
                           % (who, t.device if torch.is_tensor(t) else type(t).__name__))
    if t.dtype != dtype:
        raise RuntimeError("%s: expected a %s tensor, got %s" % (who, dtype, t.dtype))
    if t.dim() != 3 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError("%s: expected a (X, Y, Z) tensor%s, got shape %s"
                           % (who, "" if shape is None else " of shape %s" % (tuple(shape),), tuple(t.shape)))
    return t.contiguous()


def strip_starts(gm, h):
    """int32 device tensor [Z, Y-h+1]: for every slice and every row offset row0 the first column of the strip row0 .. row0+h-1
    that holds a template value > 0, -1 for an empty strip.  `gm` is a float32 (X, Y, Z) device tensor without negative values
    (checked once here): only then do the reference's `sum() == 0` and `sum(0) > 0` mean "any value > 0"."""
    gm = _require("strip_starts", gm, torch.float32)
    if not bool((gm >= 0).all()):
        raise ValueError("strip_starts: the template holds a negative or NaN value; the reference's strip sums need a non-negative one")
    x, y, z = gm.shape
    out = torch.empty((z, max(y - int(h) + 1, 0)), dtype=torch.int32, device=gm.device)
    _lib.check(_lib.lib().mri3d_strip_starts_f32(_ptr(gm), x, y, z, int(h), _ptr(out), _stream()), "strip_starts")
    return out


def _mid(shape, w):
    mid = shape[0] // 2 - w
    if mid < 1:
        raise ValueError("a patch width of %d leaves no middle patch in %d columns (X//2 - w < 1)" % (w, shape[0]))
    return mid


def _strip_patches(z, row0, start, x, w, mid):
    """The reference's patches of one non-empty strip, in its order, as (kind, (z, row0, col0))."""
    if start == 0:
        raise ValueError("slice %d, rows %d..: the template starts in column 0 (the reference asserts start_idx != 0)" % (z, row0))
    out = []
    if start < mid:
        out += [(0, (z, row0, start)), (3, (z, row0, x - start - w))]
    return out + [(1, (z, row0, mid)), (2, (z, row0, x - mid - w))]


def _check_table(table, shape, h, w):
    x, y, z = shape
    t = np.asarray(table).reshape(-1, 3)
    bad = (t[:, 0] < 0) | (t[:, 0] >= z) | (t[:, 1] < 0) | (t[:, 1] > y - h) | (t[:, 2] < 0) | (t[:, 2] > x - w)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError("patch %d = (z %d, row0 %d, col0 %d) of size %d x %d leaves the %s volume" % ((i,) + tuple(t[i]) + (h, w, (x, y, z))))


def patch_table(starts, shape, h, w, last_row=None, with_cells=False):
    """The reference's base grid (patch_utils.py:142-191) as host integers: int32 [P, 3] rows (z, row0, col0) in its order — slice,
    then strip j = 0, h, 2h, ..., then [side, side mirrored if start < mid], middle, middle mirrored.
    starts: [Z, Y-h+1] integers as `strip_starts` gives them (host array or tensor).  last_row: [Z] integers, the last row of
    each slice that holds a template value > 0 (-1: none); needed only where Y is no multiple of h, to see whether the short last
    strip is empty.  ValueError for a non-empty strip with start == 0 (the reference asserts) and for a non-empty short last strip
    (the reference's concatenate fails there).  with_cells: also return int64 [P], the flat index kind*R*Z + (row0//h)*Z + z of
    every patch in a [4, R, Z] patch map, R = Y // h."""
    x, y, z = (int(s) for s in shape)
    h, w = int(h), int(w)
    starts = np.asarray(starts.cpu() if torch.is_tensor(starts) else starts)
    if h < 1 or w < 1 or y < h or starts.shape != (z, y - h + 1):
        raise ValueError("patch_table: starts of shape %s are not the [Z, Y-h+1] table of a %s volume with h = %d" % (starts.shape, (x, y, z), h))
    mid = _mid((x, y, z), w)
    r = y // h
    if y % h:
        if last_row is None:
            raise ValueError("patch_table: Y = %d is no multiple of h = %d; give last_row to tell whether the short last strip is empty" % (y, h))
        last_row = np.asarray(last_row.cpu() if torch.is_tensor(last_row) else last_row)
        full = np.flatnonzero(last_row >= r * h)
        if full.size:
            raise ValueError("slice %d: the short last strip (rows %d..%d) is not empty; the reference cannot stack its patches"
                             % (int(full[0]), r * h, y - 1))
    rows, cells = [], []
    for i in range(z):
        for j in range(r):
            start = int(starts[i, j * h])
            if start < 0:
                continue
            for kind, row in _strip_patches(i, j * h, start, x, w, mid):
                rows.append(row)
                cells.append((kind * r + j) * z + i)
    table = np.asarray(rows, dtype=np.int32).reshape(-1, 3)
    _check_table(table, (x, y, z), h, w)
    return (table, np.asarray(cells, dtype=np.int64)) if with_cells else table


def shifted_table(starts, shape, h, w, last_row=None):
    """The candidates of the reference's "upsampling" (patch_utils.py:78-137) as host integers [Q, 3]: for k = 1 .. h-1, slice,
    j in range(0, Y-h, h), the patches of the strip row0 = k + j, in the reference's order.  The reference keeps those whose label
    is true.  A shifted strip that runs past the last row must be empty (ValueError otherwise, as in `patch_table`)."""
    x, y, z = (int(s) for s in shape)
    h, w = int(h), int(w)
    starts = np.asarray(starts.cpu() if torch.is_tensor(starts) else starts)
    mid = _mid((x, y, z), w)
    if last_row is not None:
        last_row = np.asarray(last_row.cpu() if torch.is_tensor(last_row) else last_row)
    rows = []
    for k in range(1, h):
        for i in range(z):
            for j in range(0, y - h, h):
                row0 = k + j
                if row0 > y - h:     # a strip cut short by the end of the slice
                    if last_row is None:
                        raise ValueError("shifted_table: Y = %d is no multiple of h = %d; give last_row" % (y, h))
                    if last_row[i] >= row0:
                        raise ValueError("slice %d: the shifted strip at row %d runs past the last row and is not empty; the "
                                         "reference cannot stack its patches" % (i, row0))
                    continue
                start = int(starts[i, row0])
                if start >= 0:
                    rows += [row for _, row in _strip_patches(i, row0, start, x, w, mid)]
    table = np.asarray(rows, dtype=np.int32).reshape(-1, 3)
    _check_table(table, (x, y, z), h, w)
    return table


def work_order(table):
    """int32 permutation that sorts a patch table by (row0, col0, z): patches that read neighbouring elements of the volume become
    neighbours in the order the gather kernel works in."""
    t = np.asarray(table).reshape(-1, 3)
    return np.lexsort((t[:, 0], t[:, 2], t[:, 1])).astype(np.int32)


def _device_table(table, device):
    return torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(device)


def mirror_patches(volume, table, h, w, channels_last=False, order=None, out=None):
    """Patches (P, 2, h, w) of a float32 (X, Y, Z) device volume for a DEVICE int32 table [P, 3] whose rows lie inside the volume
    (`patch_table` checks its own; `_check_table` any other).  channels_last: the same logical shape over [p][i][t][channel]
    memory (torch.channels_last), which the convolutions read without a layout copy.  A pure copy: bit-exact."""
    volume = _require("mirror_patches", volume, torch.float32)
    x, y, z = volume.shape
    p = int(table.shape[0])
    if table.dtype != torch.int32 or not table.is_cuda or table.dim() != 2 or table.shape[1] != 3 or not table.is_contiguous():
        raise RuntimeError("mirror_patches: the table must be a contiguous int32 [P, 3] device tensor")
    if order is not None and (order.dtype != torch.int32 or not order.is_cuda or order.numel() != p or not order.is_contiguous()):
        raise RuntimeError("mirror_patches: the order must be a contiguous int32 [P] device tensor")
    if out is None:
        out = torch.empty((p, h, w, 2) if channels_last else (p, 2, h, w), dtype=torch.float32, device=volume.device)
    elif out.dtype != torch.float32 or out.numel() != p * 2 * h * w or not out.is_contiguous() or out.device != volume.device:
        raise RuntimeError("mirror_patches: out must be a contiguous float32 buffer of %d elements on the volume's device" % (p * 2 * h * w))
    if p:
        _lib.check(_lib.lib().mri3d_mirror_patches_f32(_ptr(volume), x, y, z, _ptr(table), _ptr(order), p, int(h), int(w),
                                                       1 if channels_last else 0, _ptr(out), _stream()), "mirror_patches")
    out = out.view((p, h, w, 2) if channels_last else (p, 2, h, w))
    return out.permute(0, 3, 1, 2) if channels_last else out


def mirror_patch_labels(mask, table, h, w):
    """uint8 [P]: 1 where any voxel of the uint8 (X, Y, Z) device mask lies under channel 0 of the patch."""
    mask = _require("mirror_patch_labels", mask, torch.uint8)
    x, y, z = mask.shape
    p = int(table.shape[0])
    if table.dtype != torch.int32 or not table.is_cuda or table.dim() != 2 or table.shape[1] != 3 or not table.is_contiguous():
        raise RuntimeError("mirror_patch_labels: the table must be a contiguous int32 [P, 3] device tensor")
    out = torch.empty(p, dtype=torch.uint8, device=mask.device)
    if p:
        _lib.check(_lib.lib().mri3d_mirror_patch_labels_u8(_ptr(mask), x, y, z, _ptr(table), p, int(h), int(w), _ptr(out), _stream()),
                   "mirror_patch_labels")
    return out


class PatchPlan:
    """What the template decides, made once: the strip starts, the base grid's table (host and device), the order the gather
    works in and every patch's cell in the [4, R, Z] patch map.  `gm` is the (X, Y, Z) template on the device (any real dtype)."""

    def __init__(self, gm, h=16, w=32):
        if not torch.is_tensor(gm) or not gm.is_cuda:
            raise RuntimeError("PatchPlan runs only on a ROCm device tensor (got %s); there is no CPU fallback"
                               % (gm.device if torch.is_tensor(gm) else type(gm).__name__))
        self.h, self.w = int(h), int(w)
        self.shape = tuple(int(s) for s in gm.shape)
        self.device = gm.device
        gm = gm.to(torch.float32)
        x, y, z = self.shape
        self.mid = _mid(self.shape, self.w)
        self.starts = strip_starts(gm, self.h)
        self.starts_host = self.starts.cpu().numpy()
        self.last_row = None
        if y % self.h:
            rows = strip_starts(gm, 1).cpu().numpy() >= 0                      # [Z, Y]: row r of slice z holds a value > 0
            self.last_row = np.where(rows.any(1), y - 1 - rows[:, ::-1].argmax(1), -1)
        self.strips = y // self.h
        self.table_host, self.cells_host = patch_table(self.starts_host, self.shape, self.h, self.w, self.last_row, with_cells=True)
        self.table = _device_table(self.table_host, self.device)
        self.order = torch.from_numpy(work_order(self.table_host)).to(self.device)
        self.cells = torch.from_numpy(self.cells_host).to(self.device)
        # the [Z, R] starts of the base strips, as the paint kernel reads them
        self.base_starts = self.starts[:, ::self.h][:, :self.strips].contiguous()

    def __len__(self):
        return int(self.table_host.shape[0])

    def patches(self, volume, channels_last=False):
        _require("PatchPlan.patches", volume, torch.float32, self.shape)
        return mirror_patches(volume, self.table, self.h, self.w, channels_last, self.order)


def _plan(gm, h, w):
    return gm if isinstance(gm, PatchPlan) else PatchPlan(gm, h, w)


def get_only_patches(volume, gm, h=16, w=32, channels_last=False):
    """patch_utils.py:142-191 on the device: float32 (P, 2, h, w).  `gm`: the template tensor, or a `PatchPlan` of it."""
    return _plan(gm, h, w).patches(volume, channels_last)


def get_all_patches_and_labels(volume, gm, mask, h=16, w=32, channels_last=False):
    """patch_utils.py:17-140 on the device: the base grid with its labels, then the reference's "upsampling" — of every strip
    shifted by k = 1 .. h-1 rows only the patches whose label is true.  Returns (patches float32 (P, 2, h, w), labels bool [P]).
    The labels of the base grid and of all candidates come from one launch, the kept rows are picked on the host (one bool copy)
    and all patches come from one gather."""
    plan = _plan(gm, h, w)
    mask = _require("get_all_patches_and_labels", mask, torch.uint8, plan.shape)
    _require("get_all_patches_and_labels", volume, torch.float32, plan.shape)
    shifted = shifted_table(plan.starts_host, plan.shape, plan.h, plan.w, plan.last_row)
    both = np.concatenate([plan.table_host, shifted])
    labels = mirror_patch_labels(mask, _device_table(both, plan.device), plan.h, plan.w).cpu().numpy().astype(bool)
    n = len(plan)
    keep = np.concatenate([np.ones(n, dtype=bool), labels[n:]])
    table = np.ascontiguousarray(both[keep])
    order = torch.from_numpy(work_order(table)).to(plan.device)
    patches = mirror_patches(volume, _device_table(table, plan.device), plan.h, plan.w, channels_last, order)
    return patches, torch.from_numpy(labels[keep]).to(plan.device)


def min_max_normalize(volume):
    """(v - min) / (max - min) of a float32 device volume (patch_utils.py:196): the two extremes are order statistics from the
    device, the map is the float64 one-segment `mri3d_piecewise_linear_f32`."""
    import ctypes
    from ..classification.preprocessing import order_statistics
    if not volume.is_cuda or volume.dtype != torch.float32:
        raise RuntimeError("min_max_normalize: needs a float32 ROCm device tensor (got %s on %s); there is no CPU fallback"
                           % (volume.dtype, volume.device))
    data = volume.contiguous()
    lo, hi = (float(v) for v in order_statistics(data, [0, data.numel() - 1]).cpu().numpy().astype(np.float64))
    slope = np.array([1.0 / (hi - lo)], dtype=np.float64)
    intercept = np.array([-lo / (hi - lo)], dtype=np.float64)
    out = torch.empty_like(data)
    as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _lib.check(_lib.lib().mri3d_piecewise_linear_f32(_ptr(data), _ptr(out), data.numel(), None, as_p(slope), as_p(intercept), 1,
                                                     _stream()), "piecewise_linear")
    return out


def get_image_patches(volume, gm, mask=None, h=16, w=32, channels_last=False):
    """patch_utils.py:193-205 without the NIfTI reading: min-max normalise the volume, then all patches and labels (with a
    mask, taken as `mask > 0`) or only the base grid's patches with all-false labels (without one)."""
    plan = _plan(gm, h, w)
    target = min_max_normalize(volume.to(torch.float32))
    if mask is not None:
        return get_all_patches_and_labels(target, plan, (mask > 0).to(torch.uint8), channels_last=channels_last)
    patches = plan.patches(target, channels_last)
    return patches, torch.zeros(patches.shape[0], dtype=torch.bool, device=patches.device)
