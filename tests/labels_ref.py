"""References of the label path (csrc/labels.hip), all on the CPU: the id-remap rule and the confusion matrix in numpy, and the
softmax-Dice loss against a class map with its gradient in torch (float64 by default), written with an explicit one-hot target
whose rows are zero for labels >= C."""
import numpy as np
import torch

LIST_FCD = [8, 10, 11, 12, 13, 16, 17, 18, 26, 47, 49, 50, 51, 52, 53, 54, 58, 85, 251, 252, 253, 254, 255]

# values at which the rule could go wrong (floats; integer dtypes take those they can hold)
EDGE_VALUES = [float("nan"), float("inf"), float("-inf"), -1.0, -0.0, 0.0, 0.5, 1.0, 255.0, 256.0, 999.0, 999.5, 1000.0, 1000.5,
               65535.0, 65535.5, 65536.0, 70000.0, 3.0e9]


def remap_ref(v, lut, above, other, out_dtype=np.uint8):
    """v >= len(lut) -> above; v an integer in [0, len(lut)) -> lut[v]; anything else (negative, fractional, NaN, -inf) -> other."""
    v, lut = np.asarray(v), np.asarray(lut, dtype=np.uint8)
    n = lut.shape[0]
    if np.issubdtype(v.dtype, np.integer):
        w = v.astype(np.int64)
        over = w >= n
        inside = (w >= 0) & ~over
    else:
        with np.errstate(invalid="ignore"):
            over = v >= n
            inside = ~over & (v >= 0) & (v == np.floor(v))
        w = np.where(inside, v, 0).astype(np.int64)
    idx = np.where(inside, w, 0)
    return np.where(over, above, np.where(inside, lut[idx], other)).astype(out_dtype)


def fcd_luts():
    """(first sample's table, the other samples' table) of the reference's binarisation: above = 1, other = 0."""
    plain = np.zeros(1000, np.uint8)
    plain[1] = 1
    first = plain.copy()
    first[LIST_FCD] = 1
    return first, plain


def binarise_ref(targets):
    """prepare_batch's rule on a (N, ...) array, as remaps: LIST_FCD counts for the first sample only."""
    first, plain = fcd_luts()
    out = np.empty(targets.shape, targets.dtype)
    for k in range(targets.shape[0]):
        out[k] = remap_ref(targets[k], first if k == 0 else plain, 1, 0, targets.dtype)
    return out


def confusion_ref(pred, gt, classes):
    """(conf[g, p] = #(gt == g and pred == p) as int64 (C, C), #(gt >= C or pred >= C))."""
    pred, gt = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(gt).reshape(-1).astype(np.int64)
    ok = (pred < classes) & (gt < classes)
    conf = np.bincount(gt[ok] * classes + pred[ok], minlength=classes * classes).reshape(classes, classes)
    return conf.astype(np.int64), int((~ok).sum())


def class_scores_ref(conf):
    """Per-class Dice = 2 tp / (|gt| + |pred|) and IoU = tp / |gt or pred| in float64; NaN where the denominator is 0."""
    conf = np.asarray(conf, dtype=np.float64)
    tp, sg, sp = np.diag(conf), conf.sum(1), conf.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(sg + sp > 0, 2 * tp / (sg + sp), np.nan), np.where(sg + sp - tp > 0, tp / (sg + sp - tp), np.nan)


def one_hot(labels, classes, dtype=torch.float64):
    """(N, D, H, W) or (N, 1, D, H, W) integer labels -> (N, C, D, H, W); a label >= C has a zero row."""
    labels = labels.reshape(labels.shape[0], *labels.shape[-3:]).long()
    return torch.stack([(labels == c).to(dtype) for c in range(classes)], 1)


def dice_index_loss(logits, labels, eps=1e-9):
    """mean_{n,c} (1 - 2 tp / (sum_p + sum_g + eps)) with g_c = [labels == c], in the dtype of `logits` (N, C, D, H, W)."""
    g = one_hot(labels, logits.shape[1], logits.dtype)
    p = torch.softmax(logits, dim=1)
    dims = (2, 3, 4)
    tp, sp, sg = (p * g).sum(dims), p.sum(dims), g.sum(dims)
    return (1 - 2 * tp / (sp + sg + eps)).mean()


def dice_index_ref(logits, labels, eps=1e-9, dtype=torch.float64):
    """(loss, gradient) of `dice_index_loss` in `dtype` for logits given in any storage type."""
    z = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = dice_index_loss(z, labels, eps)
    loss.backward()
    return loss.detach(), z.grad.detach()
