"""Host reference of the connected-components family (csrc/components.hip, ops.label_components / component_stats /
select_components, segmentation/components.py), and the comparison the GPU suite uses.

Labels: scipy.ndimage.label with generate_binary_structure(3, 1 | 2 | 3) for 6 | 18 | 26; its numbering (ids in the order of each
component's first voxel in C-order scan) is the contract, so the comparison is element for element, with no renumbering.  With
by_value the per-value labellings are merged and renumbered by first voxel.  Statistics by np.bincount and np.minimum.at /
np.maximum.at; the lesion scores restated from their definition.  `flood_label` is a brute-force flood fill that tests/test_components.py
holds this module against on tiny volumes."""
import numpy as np
from scipy import ndimage

RANK = {6: 1, 18: 2, 26: 3}


def structure(connectivity):
    return ndimage.generate_binary_structure(3, RANK[connectivity])


def as3d(a):
    a = np.asarray(a)
    return a.reshape((1,) * (3 - a.ndim) + a.shape)


def renumber_by_first_voxel(labels):
    """Ids 1..K in the order of each id's first voxel in C order (0 stays 0)."""
    flat = labels.ravel()
    ids, first = np.unique(flat, return_index=True)
    first, ids = first[ids != 0], ids[ids != 0]
    table = np.zeros(int(flat.max()) + 1 if flat.size else 1, dtype=np.int32)
    table[ids[np.argsort(first)]] = np.arange(1, ids.size + 1, dtype=np.int32)
    return table[flat].reshape(labels.shape), int(ids.size)


def label(mask, connectivity, by_value=False):
    """(int32 labels of mask's shape, K)."""
    m = as3d(mask)
    st = structure(connectivity)
    if not by_value:
        lab, k = ndimage.label(m != 0, structure=st)
        return lab.astype(np.int32).reshape(np.shape(mask)), int(k)
    merged = np.zeros(m.shape, dtype=np.int64)
    base = 0
    for v in np.unique(m):
        if v == 0:
            continue
        lab, k = ndimage.label(m == v, structure=st)
        merged += np.where(lab > 0, lab + base, 0)
        base += k
    out, k = renumber_by_first_voxel(merged)
    return out.astype(np.int32).reshape(np.shape(mask)), k


def flood_label(mask, connectivity, by_value=False):
    """Brute force: scan in C order, flood-fill every unlabelled foreground voxel with the next id."""
    m = as3d(mask)
    key = m.astype(np.int64) if by_value else (m != 0).astype(np.int64)
    offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
            if 0 < abs(a) + abs(b) + abs(c) <= RANK[connectivity]]
    lab = np.zeros(m.shape, dtype=np.int32)
    k = 0
    for start in np.ndindex(*m.shape):
        if key[start] == 0 or lab[start]:
            continue
        k += 1
        lab[start] = k
        stack = [start]
        while stack:
            z, y, x = stack.pop()
            for a, b, c in offs:
                n = (z + a, y + b, x + c)
                if all(0 <= n[i] < m.shape[i] for i in range(3)) and lab[n] == 0 and key[n] == key[start]:
                    lab[n] = k
                    stack.append(n)
    return lab.reshape(np.shape(mask)), k


def stats(labels, capacity, other=None, score=None):
    """(int64 (capacity, 8) table, float32 (capacity,) peak or None) of ids 1..capacity, with the library's values for a row no
    voxel reaches: 0, 0, d, -1, h, -1, w, -1 and -inf."""
    lab = as3d(labels)
    d, h, w = lab.shape
    flat = lab.ravel().astype(np.int64)
    use = (flat > 0) & (flat <= capacity)
    rows = flat[use] - 1
    table = np.zeros((capacity, 8), dtype=np.int64)
    table[:, 0] = np.bincount(rows, minlength=capacity)
    if other is not None:
        table[:, 1] = np.bincount(rows, weights=(as3d(other).ravel()[use] != 0), minlength=capacity).astype(np.int64)
    z, y, x = (c.ravel()[use] for c in np.indices(lab.shape))
    for col, coord, ext in ((2, z, d), (4, y, h), (6, x, w)):
        table[:, col], table[:, col + 1] = ext, -1
        np.minimum.at(table[:, col], rows, coord)
        np.maximum.at(table[:, col + 1], rows, coord)
    peak = None
    if score is not None:
        peak = np.full(capacity, -np.inf, dtype=np.float32)
        np.maximum.at(peak, rows, as3d(score).ravel()[use].astype(np.float32))
    return table, peak


def hit(labels, other_labels, other_capacity):
    """uint8 (other_capacity,): component j + 1 of other_labels shares a voxel with any labelled voxel of labels."""
    ids = np.unique(np.asarray(other_labels)[(np.asarray(labels) > 0) & (np.asarray(other_labels) > 0)])
    out = np.zeros(other_capacity, dtype=np.uint8)
    out[ids[ids <= other_capacity] - 1] = 1
    return out


def select(labels, keep):
    keep = np.asarray(keep, dtype=np.uint8)
    lab = np.asarray(labels)
    return np.where((lab >= 0) & (lab < keep.size), keep[np.clip(lab, 0, keep.size - 1)], 0).astype(np.uint8)


def remove_small(mask, min_voxels, connectivity):
    lab, k = label(mask, connectivity)
    sizes = np.bincount(lab.ravel(), minlength=k + 1)
    keep = sizes >= min_voxels
    keep[0] = False
    return keep[lab].astype(np.uint8)


def keep_largest(mask, k, connectivity):
    lab, n = label(mask, connectivity)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    order = sorted(range(n), key=lambda i: (-sizes[i], i))[:k]      # ties: the lower id
    keep = np.zeros(n + 1, dtype=bool)
    keep[[i + 1 for i in order]] = True
    return keep[lab].astype(np.uint8)


def lesion_scores(pred, gt, connectivity, min_voxels=0):
    """From the definition: a lesion is a component of gt, a cluster a component of pred with at least min_voxels voxels; a lesion is
    detected when some kept cluster shares a voxel with it, a cluster is true when it shares a voxel with gt."""
    pred, gt = np.asarray(pred) != 0, np.asarray(gt) != 0
    if min_voxels > 1:
        pred = remove_small(pred, min_voxels, connectivity) != 0
    lc, kc = label(pred, connectivity)
    lg, kg = label(gt, connectivity)
    lesion_sizes = np.array([(lg == j).sum() for j in range(1, kg + 1)], dtype=np.int64)
    cluster_sizes = np.array([(lc == j).sum() for j in range(1, kc + 1)], dtype=np.int64)
    cluster_overlap = np.array([((lc == j) & gt).sum() for j in range(1, kc + 1)], dtype=np.int64)
    detected = sum(1 for j in range(1, kg + 1) if ((lg == j) & pred).any())
    true = int((cluster_overlap > 0).sum())
    nan = float("nan")
    return {"n_lesions": kg, "n_clusters": kc, "lesions_detected": detected, "clusters_true": true, "clusters_false": kc - true,
            "sensitivity": detected / kg if kg else nan, "precision": true / kc if kc else nan, "lesion_sizes": lesion_sizes,
            "cluster_sizes": cluster_sizes, "cluster_overlap": cluster_overlap}


def rank_clusters(mask, score, connectivity, top_k=None):
    lab, k = label(mask, connectivity)
    table, peak = stats(lab, max(k, 1), score=score)
    order = sorted(range(k), key=lambda i: (-peak[i], i))
    order = np.array(order[:top_k] if top_k is not None else order, dtype=np.int64)
    return {"ids": order + 1, "sizes": table[order, 0], "peaks": peak[order]}


# ---------------------------------------------------------------- the comparison (exact; no renumbering)
def assert_same_labelling(got_labels, got_count, want_labels, want_count, what=""):
    got_labels, want_labels = np.asarray(got_labels), np.asarray(want_labels)
    assert got_labels.dtype == np.int32, "%s: labels are %s, not int32" % (what, got_labels.dtype)
    assert got_labels.shape == want_labels.shape, "%s: shape %s vs %s" % (what, got_labels.shape, want_labels.shape)
    assert int(got_count) == int(want_count), "%s: %d components, the reference has %d" % (what, int(got_count), int(want_count))
    bad = np.argwhere(got_labels != want_labels)
    assert bad.size == 0, "%s: %d voxels differ, first at %s: %d vs %d" % (
        what, len(bad), tuple(bad[0]), got_labels[tuple(bad[0])], want_labels[tuple(bad[0])])


def assert_same_tables(got, want, what=""):
    """got, want: dicts of arrays (stats, peak, hit, ...); every key of want, bit for bit."""
    for k, w in want.items():
        g = np.ascontiguousarray(got[k])
        w = np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, "%s[%s]: %s %s vs %s %s" % (what, k, g.dtype, g.shape, w.dtype, w.shape)
        same = g.view(np.uint8).reshape(-1) == w.view(np.uint8).reshape(-1) if g.size else np.ones(0, bool)
        if not same.all():
            bad = np.argwhere(g != w)
            first = tuple(bad[0]) if len(bad) else "(bits)"
            raise AssertionError("%s[%s]: differs, first at %s: %s vs %s" % (what, k, first, g[first] if len(bad) else "", w[first] if len(bad) else ""))


def assert_same_scores(got, want, what=""):
    assert set(got) == set(want), (set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            assert np.asarray(g).dtype == w.dtype and np.array_equal(np.asarray(g), w), "%s[%s]: %s vs %s" % (what, k, g, w)
        elif isinstance(w, float):
            assert (np.isnan(g) and np.isnan(w)) or g == w, "%s[%s]: %r vs %r" % (what, k, g, w)
        else:
            assert type(g) is int and g == w, "%s[%s]: %r vs %r" % (what, k, g, w)
