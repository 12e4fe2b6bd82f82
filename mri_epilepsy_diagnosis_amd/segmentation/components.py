"""Connected components of device masks: lesion-wise detection scores, cluster ranking and the usual mask clean-up.

A detector of focal cortical dysplasia is judged per lesion: was the lesion hit by any predicted cluster, how many clusters are
false alarms, how large they are, which one ranks highest.  The masks this package produces (ops.argmax_mask, the Monte-Carlo
mask of mc_finalize, the class maps of remap_labels, FCDMaskGenerator.get_mask) are device tensors; here their components are
labelled, measured and filtered where they lie (ops.label_components / component_stats / select_components, csrc/components.hip)
with scipy.ndimage.label's numbering, and only the per-component tables (a few numbers per cluster) cross to the host.

Connectivity is 6, 18 or 26 (scipy's 1, 2, 3 are accepted); the default everywhere is 26, the usual choice for lesion counting.
"""
import collections

import torch

from .. import ops

Components = collections.namedtuple("Components", "labels count sizes boxes overlap peak hit")
Components.__doc__ = """labels: int32 device volume, 0 = background, ids 1..count by first voxel in C order.  count: int (read once
from the device to size the tables).  Device tables with row id - 1: sizes int64 (count,), boxes int64 (count, 6) = inclusive
dmin, dmax, hmin, hmax, wmin, wmax, overlap int64 (count,) voxels inside `other` (None without it), peak float32 (count,) maximum
of `score` (None without it), hit uint8 (components of `other`,) = 1 where that component of `other` is touched by any component
here (None without `other`)."""


def _as_mask(who, mask):
    if not torch.is_tensor(mask) or not mask.is_cuda:
        raise RuntimeError("%s runs only on ROCm device tensors (got %s); there is no CPU fallback"
                           % (who, mask.device if torch.is_tensor(mask) else type(mask).__name__))
    if mask.dtype == torch.bool:
        return mask.view(torch.uint8)
    if mask.dtype != torch.uint8:
        raise RuntimeError("%s: the mask must be uint8 or bool, got %s" % (who, mask.dtype))
    return mask


def components(mask, connectivity=26, by_value=False, other=None, score=None, _other_labelled=None):
    """Label `mask` and measure its components -> Components.  other: a second uint8 / bool mask of the same shape (the ground
    truth when `mask` is a prediction): `overlap` counts each component's voxels inside it and `hit` says which of ITS components
    (same connectivity) are touched.  score: a float32 volume, whose maximum per component is `peak`."""
    who = "components"
    mask = _as_mask(who, mask)
    labels, count = ops.label_components(mask, connectivity, by_value)
    other_labels, k_other = None, 0
    if other is not None:
        other = _as_mask(who, other)
        if _other_labelled is not None:       # lesion_scores has labelled `other` already
            (other_labels, k_other), k = _other_labelled, int(count)
        else:
            other_labels, k_other = ops.label_components(other, connectivity)
            k, k_other = (int(v) for v in torch.stack((count, k_other)).tolist())
    else:
        k = int(count)
    dev = mask.device
    hit = None if other is None else torch.zeros(k_other, dtype=torch.uint8, device=dev)
    if k == 0:
        return Components(labels, 0, torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros((0, 6), dtype=torch.int64, device=dev),
                          None if other is None else torch.zeros(0, dtype=torch.int64, device=dev),
                          None if score is None else torch.zeros(0, dtype=torch.float32, device=dev), hit)
    with_hit = other is not None and k_other > 0
    res = ops.component_stats(labels, k, other=other, other_labels=other_labels if with_hit else None, score=score,
                              other_capacity=k_other if with_hit else None)
    stats = res["stats"]
    return Components(labels, k, stats[:, 0], stats[:, 2:8], None if other is None else stats[:, 1], res.get("peak"),
                      res["hit"] if with_hit else hit)


def _keep_table(flags):
    """keep[0] = 0 for the background, keep[id] = flags[id - 1]; built on the device."""
    keep = torch.zeros(flags.numel() + 1, dtype=torch.uint8, device=flags.device)
    keep[1:] = flags.to(torch.uint8)
    return keep


def remove_small(mask, min_voxels, connectivity=26):
    """The uint8 0/1 mask of the components of `mask` with at least `min_voxels` voxels."""
    c = components(mask, connectivity)
    return ops.select_components(c.labels, _keep_table(c.sizes >= int(min_voxels)))


def keep_largest(mask, k=1, connectivity=26):
    """The uint8 0/1 mask of the `k` largest components of `mask`; among equal sizes the lower id (the earlier first voxel) wins."""
    c = components(mask, connectivity)
    flags = torch.zeros(c.count, dtype=torch.uint8, device=c.labels.device)
    if c.count and int(k) > 0:
        order = torch.sort(c.sizes, descending=True, stable=True).indices   # stable: ties stay in id order
        flags[order[:int(k)]] = 1
    return ops.select_components(c.labels, _keep_table(flags))


def _ratio(a, b):
    return a / b if b else float("nan")


def lesion_scores(pred, gt, connectivity=26, min_voxels=0):
    """Lesion-wise scores of a predicted mask against the ground truth, both uint8 / bool device masks of one shape.  A lesion is a
    component of `gt`, a cluster a component of `pred` (after dropping clusters under `min_voxels`).  A lesion is detected when any
    cluster shares a voxel with it; a cluster is true when it shares a voxel with `gt`, else false.  Returns a dict of host values:
      n_lesions, n_clusters, lesions_detected, clusters_true, clusters_false   ints
      sensitivity = lesions_detected / n_lesions, precision = clusters_true / n_clusters   (NaN where the denominator is 0)
      lesion_sizes, cluster_sizes, cluster_overlap   int64 arrays in id order (cluster_overlap: the cluster's voxels inside gt)"""
    who = "lesion_scores"
    pred, gt = _as_mask(who, pred), _as_mask(who, gt)
    if pred.shape != gt.shape:
        raise RuntimeError("%s: shapes differ %s vs %s" % (who, tuple(pred.shape), tuple(gt.shape)))
    if int(min_voxels) > 1:
        pred = remove_small(pred, min_voxels, connectivity)
    lesions = components(gt, connectivity)
    clusters = components(pred, connectivity, other=gt, _other_labelled=(lesions.labels, lesions.count))
    small = torch.cat((clusters.sizes, clusters.overlap, lesions.sizes, clusters.hit.to(torch.int64))).cpu().numpy()
    kc, kl = clusters.count, lesions.count
    cluster_sizes, cluster_overlap, lesion_sizes, hit = small[:kc], small[kc:2 * kc], small[2 * kc:2 * kc + kl], small[2 * kc + kl:]
    detected, true = int(hit.sum()), int((cluster_overlap > 0).sum())
    return {"n_lesions": kl, "n_clusters": kc, "lesions_detected": detected, "clusters_true": true, "clusters_false": kc - true,
            "sensitivity": _ratio(detected, kl), "precision": _ratio(true, kc), "lesion_sizes": lesion_sizes,
            "cluster_sizes": cluster_sizes, "cluster_overlap": cluster_overlap}


def rank_clusters(mask, score, connectivity=26, top_k=None):
    """The components of `mask` ordered by the peak of the float32 volume `score` inside them, descending, then by id: a dict of
    device tensors "ids" (int64, 1-based), "sizes" (int64), "peaks" (float32), the first `top_k` of them.  `score` is, for instance,
    the Monte-Carlo mean probability or the mutual information of uncertainty.mc_predict."""
    c = components(mask, connectivity, score=score)
    order = torch.sort(c.peak, descending=True, stable=True).indices
    if top_k is not None:
        order = order[:int(top_k)]
    return {"ids": order + 1, "sizes": c.sizes[order], "peaks": c.peak[order]}
