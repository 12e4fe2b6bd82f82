"""CPU references of the cross-entropy / focal family (csrc/ce_loss.hip), all in torch:

  ce_loss / ce_ref            the loss from its definition and its gradient by autograd, float64 by default, float32 for the error
                              measure e32 of the GPU suite
  compound_ref                dice_weight * labels_ref.dice_index_loss + ce_weight * ce_loss, the same way
  ce_grad_closed              the closed-form gradient the kernel implements
  emulate                     the kernel's float32 expressions in the kernel's order (sums in double, as its lanes keep them), with
                              optional planted mistakes: what a wrong kernel would return
  bound / inside              the GPU suite's acceptance rule, shared with tests/test_ce_ref.py

  logp_y = z_y - max z - log sum_j exp(z_j - max z),  pt = softmax(z)_y
  l_v    = -w_y (1 - pt)^gamma logp_y   (0 for an ignored voxel: label >= C)
  CE     = sum_v l_v / sum_v w_y        (0 when no voxel counts)
"""
import torch

import labels_ref

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
MISTAKES = ("count_denominator", "weight_missing_in_gradient", "gamma_term_dropped", "ignored_counted", "log_pt", "weights_swapped")


def _flat_labels(labels):
    return labels.reshape(labels.shape[0], *labels.shape[-3:]).long()


def ce_loss(logits, labels, weight=None, gamma=0.0):
    """The definition, in the dtype of `logits` (N, C, D, H, W); labels uint8 (N, D, H, W) or (N, 1, D, H, W)."""
    C = logits.shape[1]
    lab = _flat_labels(labels)
    valid = lab < C
    y = torch.where(valid, lab, torch.zeros_like(lab))
    w = torch.ones(C, dtype=logits.dtype) if weight is None else weight.to(logits.dtype)
    logp = torch.log_softmax(logits, dim=1).gather(1, y[:, None])[:, 0]
    wy = torch.where(valid, w[y], torch.zeros((), dtype=logits.dtype))
    lv = -wy * logp
    if gamma != 0.0:
        lv = lv * (1.0 - logp.exp()).clamp_min(0.0) ** gamma
    den = wy.sum()
    if float(den) == 0.0:
        return (lv * 0.0).sum()
    return lv.sum() / den


def ce_ref(logits, labels, weight=None, gamma=0.0, dtype=F64):
    """(loss, gradient) of ce_loss in `dtype` for logits given in any storage type."""
    return compound_ref(logits, labels, 0.0, 1.0, weight, gamma, dtype=dtype)


def compound_ref(logits, labels, dice_weight=1.0, ce_weight=1.0, weight=None, gamma=0.0, eps=1e-9, dtype=F64):
    z = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = ce_weight * ce_loss(z, labels, weight, gamma)
    if dice_weight != 0.0:
        loss = loss + dice_weight * labels_ref.dice_index_loss(z, labels, eps)
    loss.backward()
    return loss.detach(), z.grad.detach()


def ce_grad_closed(logits, labels, weight=None, gamma=0.0):
    """dCE/dz_j(v) = (w_y / sum w) [(1 - pt)^gamma - gamma pt (1 - pt)^(gamma - 1) logp_y] (p_j - [j == y]) in float64."""
    z = logits.detach().double()
    C = z.shape[1]
    lab = _flat_labels(labels)
    valid = lab < C
    y = torch.where(valid, lab, torch.zeros_like(lab))
    w = torch.ones(C, dtype=F64) if weight is None else weight.double()
    p = torch.softmax(z, dim=1)
    logp = torch.log_softmax(z, dim=1).gather(1, y[:, None])[:, 0]
    pt = logp.exp()
    omp = (p.sum(1) - p.gather(1, y[:, None])[:, 0]).clamp_min(0.0)
    wy = torch.where(valid, w[y], torch.zeros((), dtype=F64))
    den = wy.sum()
    if float(den) == 0.0:
        return torch.zeros_like(z)
    slope = torch.ones_like(pt) if gamma == 0.0 else omp ** gamma - gamma * pt * omp ** (gamma - 1.0) * logp
    onehot = torch.zeros_like(z).scatter_(1, y[:, None], 1.0)
    return (wy / den * slope)[:, None] * (p - onehot)


# ------------------------------------------------------------------------------------------------ the kernel in float32
def _seq_sum(x, dim):
    """Sum along `dim` one element after the other in the tensor's dtype (a lane's class loop)."""
    parts = x.unbind(dim)
    s = parts[0].clone()
    for t in parts[1:]:
        s = s + t
    return s


def _focal_q(omp, gamma):
    if gamma == 1.0:
        return torch.ones_like(omp)
    if gamma == 2.0:
        return omp
    return omp ** (gamma - 1.0)


def emulate(logits, labels, weight=None, gamma=0.0, dice_weight=0.0, ce_weight=1.0, eps=1e-9, mistake=None):
    """(loss float32, gradient in the storage type of `logits`) as ce_loss.hip computes them: float32 per voxel, the sums over voxels
    in double, the Dice value and coefficients in float32 from the rounded sums.  `mistake`: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    if mistake == "weights_swapped":
        dice_weight, ce_weight = ce_weight, dice_weight
    z = logits.detach().to(F32)
    N, C = z.shape[:2]
    lab = _flat_labels(labels)
    valid = lab < C
    if mistake == "ignored_counted":
        lab = torch.where(valid, lab, torch.zeros_like(lab))
        valid = torch.ones_like(valid)
    y = torch.where(valid, lab, torch.zeros_like(lab))
    w = torch.ones(C, dtype=F32) if weight is None else weight.to(F32)
    onehot = torch.zeros_like(z).scatter_(1, y[:, None], 1.0) * valid[:, None].float()
    m = z.amax(1, keepdim=True)
    e = torch.exp(z - m)
    s = _seq_sum(e, 1)
    zy, ey = (z * onehot).sum(1), (e * onehot).sum(1)
    so = _seq_sum(e * (1.0 - onehot), 1)
    inv = 1.0 / s
    pt, omp = ey * inv, so * inv
    logp = torch.log(pt) if mistake == "log_pt" else (zy - m[:, 0]) - torch.log(s)
    wy = torch.where(valid, w[y], torch.zeros((), dtype=F32))
    f = torch.ones_like(omp) if gamma == 0.0 else _focal_q(omp, gamma) * omp
    lv = torch.where(valid, wy * (-f * logp), torch.zeros((), dtype=F32))
    num = lv.double().sum()
    den = valid.double().sum() if mistake == "count_denominator" else wy.double().sum()
    ce = (num / den).float() if float(den) > 0 else torch.zeros((), dtype=F32)
    invden = (1.0 / den).float() if float(den) > 0 else torch.zeros((), dtype=F32)
    # gradient of the CE part
    if gamma == 0.0:
        slope = torch.ones_like(pt)
    else:
        q = _focal_q(omp, gamma)
        slope = q * omp if mistake == "gamma_term_dropped" else q * omp - gamma * pt * q * logp
    kce = torch.tensor(ce_weight, dtype=F32) * invden
    wg = torch.ones_like(wy) if mistake == "weight_missing_in_gradient" else wy
    a = torch.where(valid, kce * wg * slope, torch.zeros((), dtype=F32))
    p = e * inv[:, None]
    pm = torch.where(onehot > 0, (-omp)[:, None].expand_as(p), p)              # p_j - [j == y], the hit without a subtraction
    grad = a[:, None] * pm
    loss = torch.tensor(ce_weight, dtype=F32) * ce
    if dice_weight != 0.0:
        dims = (2, 3, 4)
        tp, sp, sg = (p * onehot).double().sum(dims).float(), p.double().sum(dims).float(), onehot.double().sum(dims).float()
        dice = (1.0 - (2.0 * tp / (2.0 * tp + (sp - tp) + (sg - tp) + eps)).double()).mean().float()
        loss = torch.tensor(dice_weight, dtype=F32) * dice + loss
        scale = torch.tensor(dice_weight / (N * C), dtype=F32)
        dn = sp + sg + eps
        ka, kb = (-2.0 * scale / dn)[:, :, None, None, None], (2.0 * scale * tp / (dn * dn))[:, :, None, None, None]
        dp = ka * onehot + kb
        dot = _seq_sum(p * dp, 1)
        grad = grad + p * (dp - dot[:, None])
    return loss, grad.to(logits.dtype)


# ------------------------------------------------------------------------------------------------ the acceptance rule
LOSS_REL = 1e-5


def bound(g64, e32, dtype):
    """Per-element bound of the gradient's absolute error: 8 x max(e32, 2^-23 max|g64|), bf16 storage adds 2^-8 |g64|."""
    b = torch.full_like(g64, 8.0 * max(e32, 2.0 ** -23 * g64.abs().max().item()))
    return b + 2.0 ** -8 * g64.abs() if dtype == BF else b


def reference(z, lab, weight, gamma, dice_weight, ce_weight, eps=1e-9):
    """(float64 loss, float64 gradient, e32) of the stored logits; e32: how far torch's CPU float32 autograd is from float64."""
    l64, g64 = compound_ref(z, lab, dice_weight, ce_weight, weight, gamma, eps)
    _, g32 = compound_ref(z, lab, dice_weight, ce_weight, weight, gamma, eps, dtype=F32)
    return l64.item(), g64, (g32.double() - g64).abs().max().item()


def inside(loss, grad, l64, g64, e32, dtype):
    """(ok, loss error relative to |l64| (absolute when l64 == 0), worst gradient error / bound, all finite)."""
    finite = bool(torch.isfinite(grad.float()).all()) and bool(torch.isfinite(torch.as_tensor(loss)).all())
    lerr = abs(float(loss) - l64) / (abs(l64) if l64 != 0.0 else 1.0)
    worst = float("inf")
    if finite:
        err, b = (grad.double() - g64).abs(), bound(g64, e32, dtype)
        # a zero bound (nothing counts: the reference gradient is exactly 0) admits no error at all
        worst = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double()).max().item()
    return finite and lerr <= LOSS_REL and worst <= 1.0, lerr, worst, finite
