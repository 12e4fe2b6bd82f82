"""Numpy / float64-torch restatement of the detection path, written from the closed form (not from the reference's text):

  slice z of A (X, Y, Z) is B = np.rot90(A[:, :, z]), B[r, c] = A[c, Y-1-r, z]; a patch (z, row0, col0) is
  channel 0 = B[row0+i, col0+t], channel 1 = B[row0+i, X-1-col0-t]; the reference's patch kinds are col0 = start, X-start-w
  (sides, where start < mid) and mid, X-mid-w (middles), mid = X//2 - w, start the first column of the strip with a template
  value > 0.

tests/golden/detection_patches.npz pins these functions to the reference's own loops bit for bit (test_detection.py)."""
import numpy as np
import torch
import torch.nn as tnn


def strip_starts(gm, h):
    """int32 [Z, Y-h+1]: first column with any template value > 0 in rows row0 .. row0+h-1 of slice z, -1 for an empty strip."""
    x, y, z = gm.shape
    rows = np.transpose(gm > 0, (2, 1, 0))[:, ::-1, :]              # [z, r, c] = A[c, Y-1-r, z] > 0
    csum = np.concatenate([np.zeros((z, 1, x), np.int32), np.cumsum(rows, axis=1, dtype=np.int32)], axis=1)
    strip = (csum[:, h:, :] - csum[:, :y - h + 1, :]) > 0            # [z, row0, c]
    return np.where(strip.any(2), strip.argmax(2), -1).astype(np.int32)


def last_rows(gm):
    """[Z]: the last row r of each slice that holds a template value > 0, -1 for none."""
    rows = np.transpose(gm > 0, (2, 1, 0))[:, ::-1, :].any(2)
    return np.where(rows.any(1), gm.shape[1] - 1 - rows[:, ::-1].argmax(1), -1)


def strip_cols(start, x, w):
    """(kind, col0) of one non-empty strip in the reference's order."""
    mid = x // 2 - w
    side = [(0, start), (3, x - start - w)] if start < mid else []
    return side + [(1, mid), (2, x - mid - w)]


def base_table(gm, h, w):
    """(table int32 [P, 3] rows (z, row0, col0), kinds [P]) of the base grid, in the reference's order."""
    x, y, z = gm.shape
    starts = strip_starts(gm, h)
    rows, kinds = [], []
    for i in range(z):
        for j in range(0, y - h + 1, h):
            if starts[i, j] >= 0:
                for kind, col0 in strip_cols(int(starts[i, j]), x, w):
                    rows.append((i, j, col0))
                    kinds.append(kind)
    return np.asarray(rows, np.int32).reshape(-1, 3), np.asarray(kinds, np.int64)


def shifted_table(gm, h, w):
    """Candidates of the reference's upsampling: k = 1..h-1, slice, j in range(0, Y-h, h), strip row0 = k + j."""
    x, y, z = gm.shape
    starts = strip_starts(gm, h)
    rows = []
    for k in range(1, h):
        for i in range(z):
            for j in range(0, y - h, h):
                if k + j <= y - h and starts[i, k + j] >= 0:
                    rows += [(i, k + j, col0) for _, col0 in strip_cols(int(starts[i, k + j]), x, w)]
    return np.asarray(rows, np.int32).reshape(-1, 3)


def gather(vol, table, h, w):
    """(P, 2, h, w) patches of vol for a table, dtype of vol."""
    x, y, z = vol.shape
    t = np.asarray(table).reshape(-1, 3)
    zz = t[:, 0][:, None, None]
    yy = (y - 1 - t[:, 1])[:, None, None] - np.arange(h)[None, :, None]
    c0 = t[:, 2][:, None, None] + np.arange(w)[None, None, :]
    return np.stack([vol[c0, yy, zz], vol[x - 1 - c0, yy, zz]], axis=1)


def labels_of(mask, table, h, w):
    return gather(mask.astype(np.uint8), table, h, w)[:, 0].reshape(len(table), -1).any(1)


def get_only_patches(vol, gm, h, w):
    return gather(vol, base_table(gm, h, w)[0], h, w)


def get_all_patches_and_labels(vol, gm, mask, h, w):
    base = base_table(gm, h, w)[0]
    shifted = shifted_table(gm, h, w)
    keep = labels_of(mask, shifted, h, w)
    table = np.concatenate([base, shifted[keep]])
    return gather(vol, table, h, w), np.concatenate([labels_of(mask, base, h, w), np.ones(int(keep.sum()), bool)])


def vote(patch_map):
    """4-neighbour vote over the last two axes of a [4, R, S] 0/1 map, integer counts, every cell decided from the input."""
    m = (np.asarray(patch_map) != 0).astype(np.int64)
    p = np.pad(m, ((0, 0), (1, 1), (1, 1)))
    count = p[:, :-2, 1:-1] + p[:, 2:, 1:-1] + p[:, 1:-1, :-2] + p[:, 1:-1, 2:]
    out = np.asarray(patch_map).copy()
    out[count == 4] = 1
    out[count == 0] = 0
    return out


def paint(patch_map, gm, h, w):
    """uint8 (X, Y, Z) mask: the channel-0 footprint of every base-grid patch filled with its map value, in the reference's paint
    order (side, side mirrored, middle, middle mirrored), so the later one stays where two overlap."""
    x, y, z = gm.shape
    starts = strip_starts(gm, h)
    out = np.zeros((x, y, z), np.uint8)
    for i in range(z):
        for j in range(y // h):
            start = int(starts[i, j * h])
            if start < 0:
                continue
            cols = dict(strip_cols(start, x, w))
            for kind in (0, 3, 1, 2):
                if kind in cols:
                    out[cols[kind]:cols[kind] + w, y - (j + 1) * h:y - j * h, i] = patch_map[kind, j, i]
    return out


def map_of_labels(labels, gm, h, w):
    x, y, z = gm.shape
    table, kinds = base_table(gm, h, w)
    m = np.zeros((4, y // h, z), np.uint8)
    m[kinds, table[:, 1] // h, table[:, 0]] = labels
    return m


class RefConvolutionBlock(tnn.Module):
    def __init__(self, in_c, out_c, pad=0):
        super().__init__()
        self.conv = tnn.Conv2d(in_c, out_c, kernel_size=3, padding=pad)
        self.bn = tnn.BatchNorm2d(out_c)
        self.relu = tnn.ReLU()

    def forward(self, x):
        return self.relu(self.bn(self.conv(x)))


class RefPatchModel(tnn.Module):
    """The patch classifier in plain torch.nn: five valid 3x3 conv -> BatchNorm -> ReLU blocks (2, 16, 32, 64, 128, 256 channels),
    a 2x2 max-pool, flatten (NCHW order), dropout 0.4, Linear(3*11*256, 256) -> ReLU -> Linear(256, 2)."""

    def __init__(self):
        super().__init__()
        chans = (2, 16, 32, 64, 128, 256)
        self.conv_blocks = tnn.Sequential(*[RefConvolutionBlock(a, b) for a, b in zip(chans[:-1], chans[1:])], tnn.MaxPool2d(2))
        self.flatten = tnn.Flatten()
        self.dropout = tnn.Dropout(p=0.4)
        self.fc1 = tnn.Linear(3 * 11 * 256, 256)
        self.fc2 = tnn.Linear(256, 2)

    def forward(self, x):
        x = self.dropout(self.flatten(self.conv_blocks(x)))
        return self.fc2(torch.relu(self.fc1(x)))
