"""float64 reference of the norm-activation family (ops.norm_act), with the magnitudes its error bounds are stated in.

Plain torch on the CPU, no F.batch_norm: y = act(gamma * (x - mean) * invstd + beta) and its backward for statistics "batch"
(per channel over N x voxels), "instance" (per (n, c)), "group" (per (n, group of group_c channels)), "running" (given constants)
and "none" (no normalisation), activation None / "relu" / "leaky_relu" / "prelu" with one slope or one per channel.  Tensors are
logical (N, C, D, H, W) float64; for a bf16 row the caller passes the bf16-rounded values.

The bounds of tests/test_norm_parity_gpu.py are written in the unit roundoff u = 2^-24 and in magnitudes that come from THIS
reference, never from the kernel:
    M  = |gamma| * invstd * (|x| + |mean|) + |beta|             per element: the size of the terms the pre-activation is made of
    L1 sums per channel: sum |du|, sum |du| * (|x| + |mean|) * invstd, sum over the negative side of |dy| * M

`condition` moves the few inputs whose pre-activation lies within 64 * u * M of the activation's kink.  The forward kernel forms the
pre-activation as fma(x, gamma*invstd, beta - mean*gamma*invstd), the backward kernels as fma(gamma, (x - mean)*invstd, beta); both
are within 8 * u * M of the float64 value, so with the margin (8 times that) the two kernels and the reference take the same side
for every element and no element has to be left out of a gradient comparison."""
import numpy as np
import torch

U = 2.0 ** -24
KINK_MARGIN = 64.0     # in units of u * M
EPS_DEFAULT = 1e-5


def eps32(eps):
    """The geometry carries eps as a float: the kernels add exactly this value."""
    return float(np.float32(eps))


def round_bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def bf16_ulp(t):
    """Spacing of bf16 at |t| (8 significand bits), elementwise; the smallest normal's for zero."""
    a = t.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7.0)


def _bc(p, c):
    """A per-channel (or single) parameter as a (1, C, 1, 1, 1) float64 tensor."""
    p = p.detach().double().reshape(-1)
    if p.numel() == 1:
        p = p.expand(c)
    return p.reshape(1, c, 1, 1, 1)


def statistics(x, mode, eps=EPS_DEFAULT, group_c=0, running=None):
    """(mean, var, invstd, count) broadcastable against x; count = elements per statistic.  var is the biased variance."""
    n, c = x.shape[:2]
    e = eps32(eps)
    if mode == "none":
        z = torch.zeros(1, c, 1, 1, 1, dtype=torch.float64)
        return z, None, torch.ones_like(z), 0
    if mode == "running":
        rm, rv = running
        var = _bc(rv, c)
        return _bc(rm, c), var, 1.0 / torch.sqrt(var + e), 0
    if mode == "batch":
        dims, cnt = (0, 2, 3, 4), n * x[0, 0].numel()
        mean = x.mean(dims, keepdim=True)
        var = ((x - mean) ** 2).mean(dims, keepdim=True)
    elif mode == "instance":
        dims, cnt = (2, 3, 4), x[0, 0].numel()
        mean = x.mean(dims, keepdim=True)
        var = ((x - mean) ** 2).mean(dims, keepdim=True)
    elif mode == "group":
        assert group_c > 0 and c % group_c == 0
        xg = x.reshape(n, c // group_c, group_c, -1)
        cnt = xg.shape[2] * xg.shape[3]
        mg = xg.mean((2, 3), keepdim=True)
        vg = ((xg - mg) ** 2).mean((2, 3), keepdim=True)
        mean = mg.expand(-1, -1, group_c, 1).reshape(n, c, 1, 1, 1)
        var = vg.expand(-1, -1, group_c, 1).reshape(n, c, 1, 1, 1)
    else:
        raise ValueError(mode)
    return mean, var, 1.0 / torch.sqrt(var + e), cnt


def slopes(act, alpha, slope, c):
    """The negative-side slope per channel, (1, C, 1, 1, 1); None for the identity."""
    if act is None:
        return None
    if act == "relu":
        return torch.zeros(1, c, 1, 1, 1, dtype=torch.float64)
    if act == "leaky_relu":
        return torch.full((1, c, 1, 1, 1), float(np.float32(slope)), dtype=torch.float64)
    assert act == "prelu"
    return _bc(alpha, c)


def pre_activation(x, gamma, beta, mode, eps=EPS_DEFAULT, group_c=0, running=None):
    """(u64, M, mean, invstd) of x: the pre-activation and the magnitude of its terms."""
    c = x.shape[1]
    mean, _, invstd, _ = statistics(x, mode, eps, group_c, running)
    g = _bc(gamma, c) if gamma is not None else torch.ones(1, c, 1, 1, 1, dtype=torch.float64)
    b = _bc(beta, c) if beta is not None else torch.zeros(1, c, 1, 1, 1, dtype=torch.float64)
    u = g * ((x - mean) * invstd) + b
    m = g.abs() * invstd * (x.abs() + mean.abs()) + b.abs()
    return u, m, mean, invstd


def condition(x, gamma, beta, mode, act, eps=EPS_DEFAULT, group_c=0, running=None, bf16=False, max_rounds=4):
    """x with every pre-activation at least KINK_MARGIN * u * M from zero: (x', rounds, elements changed).  Offending elements are
    moved away from the kink by twice the margin (in whole bf16 ulps of the element for a bf16 row, then the result is a bf16
    value; an fp32 value otherwise) and the statistics recomputed.  Raises when `max_rounds` rounds do not suffice.  The identity
    activation has no kink: x is returned as it is."""
    if act is None:
        return x, 0, 0
    x = x.clone()
    c = x.shape[1]
    g = _bc(gamma, c) if gamma is not None else torch.ones(1, c, 1, 1, 1, dtype=torch.float64)
    changed = torch.zeros_like(x, dtype=torch.bool)
    for rounds in range(max_rounds + 1):
        u, m, mean, invstd = pre_activation(x, gamma, beta, mode, eps, group_c, running)
        bad = u.abs() < KINK_MARGIN * U * m
        if not bool(bad.any()):
            return x, rounds, int(changed.sum())
        if rounds == max_rounds:
            break
        # |du/dx| = |gamma| * invstd (the statistics move far less than the element): a step of 2 * margin * u * M / that
        need = 2.0 * KINK_MARGIN * U * m / (g.abs() * invstd)
        away = torch.where(u >= 0, 1.0, -1.0) * torch.sign(g)
        if bf16:
            ulp = bf16_ulp(x)
            step = torch.ceil(need / ulp).clamp_min(1.0) * ulp
            moved = round_bf16(x + away * step)
        else:
            moved = (x + away * need).to(torch.float32).to(torch.float64)
        x = torch.where(bad, moved, x)
        changed |= bad
    raise AssertionError("conditioning did not terminate in %d rounds: %d elements still within the margin" % (max_rounds, int(bad.sum())))


def norm_act_ref(x, dy, gamma, beta, alpha, mode, act, slope=0.01, eps=EPS_DEFAULT, group_c=0, running=None, momentum=0.1,
                 bf16=False):
    """The float64 results and magnitudes of one norm_act forward + backward as a dict (all float64, logical NCDHW or per channel):
      y, dx, dgamma, dbeta, dalpha (None without PReLU; one element for a shared slope), running_mean / running_var after the
      update ("batch" with `running` given), mean, invstd, var, u, du, xhat, S0 = sum du, S1 = sum du*xhat per statistic and channel
      ((G, C) with G = 1 or N), k0, k1, k2 of dx = k0*du - k1 - xhat*k2 (broadcastable against x; the group's for GroupNorm),
      M, l1_du, l1_dgamma, l1_dalpha (per channel; l1_dalpha summed over the channels for a shared slope), y_bf16 / dx_bf16 (bf16
      rows: the two rounded to bf16)."""
    n, c = x.shape[:2]
    training = mode in ("batch", "instance", "group")
    mean, var, invstd, cnt = statistics(x, mode, eps, group_c, running)
    g = _bc(gamma, c) if gamma is not None else torch.ones(1, c, 1, 1, 1, dtype=torch.float64)
    b = _bc(beta, c) if beta is not None else torch.zeros(1, c, 1, 1, 1, dtype=torch.float64)
    al = slopes(act, alpha, slope, c)
    xhat = (x - mean) * invstd
    u = g * xhat + b
    m = g.abs() * invstd * (x.abs() + mean.abs()) + b.abs()
    if al is None:
        pos = torch.ones_like(u, dtype=torch.bool)
        y, du = u, dy
    else:
        pos = u > 0
        y = torch.where(pos, u, al * u)
        du = torch.where(pos, dy, dy * al)
    red = (0, 2, 3, 4)
    out = dict(mean=mean, invstd=invstd, var=var, u=u, du=du, xhat=xhat, M=m, y=y, pos=pos, count=cnt)
    out["dbeta"] = du.sum(red)
    out["dgamma"] = (du * xhat).sum(red)
    scale = x.abs() + mean.abs()
    out["l1_du"] = du.abs().sum(red)
    out["l1_dgamma"] = (du.abs() * scale * invstd).sum(red)
    neg_terms = torch.where(pos, torch.zeros_like(u), dy * u)
    neg_l1 = torch.where(pos, torch.zeros_like(u), dy.abs() * m)
    if act == "prelu":
        shared = alpha.numel() == 1
        out["dalpha"] = neg_terms.sum().reshape(1) if shared else neg_terms.sum(red)
        out["l1_dalpha"] = neg_l1.sum().reshape(1) if shared else neg_l1.sum(red)
    else:
        out["dalpha"], out["l1_dalpha"] = None, None
    # sums per statistic: (G, C), G = 1 (batch and the frozen modes) or N
    per = (2, 3, 4) if mode in ("instance", "group") else red
    s0 = du.sum(per, keepdim=True)
    s1 = (du * xhat).sum(per, keepdim=True)
    out["S0"], out["S1"] = s0.reshape(-1, c), s1.reshape(-1, c)
    k0 = g * invstd
    if not training:
        k1 = k2 = torch.zeros(1, c, 1, 1, 1, dtype=torch.float64)
    elif mode == "group":
        gs0 = (g * s0).reshape(n, c // group_c, group_c).sum(2, keepdim=True).expand(-1, -1, group_c).reshape(n, c, 1, 1, 1)
        gs1 = (g * s1).reshape(n, c // group_c, group_c).sum(2, keepdim=True).expand(-1, -1, group_c).reshape(n, c, 1, 1, 1)
        k1, k2 = invstd * gs0 / cnt, invstd * gs1 / cnt
    else:
        k1, k2 = k0 * s0 / cnt, k0 * s1 / cnt
    out["k0"], out["k1"], out["k2"] = k0, k1, k2
    out["dx"] = k0 * du - k1 - xhat * k2
    out["dx_bound_scale"] = (k0 * du).abs() + k1.abs() + k2.abs() * scale * invstd
    if mode == "batch" and running is not None:
        rm, rv = (t.detach().double().reshape(-1) for t in running)
        unb = var.reshape(-1) * (cnt / (cnt - 1.0) if cnt > 1 else 1.0)
        mo = float(np.float32(momentum))
        out["running_mean"] = (1.0 - mo) * rm + mo * mean.reshape(-1)
        out["running_var"] = (1.0 - mo) * rv + mo * unb
    if bf16:
        out["y_bf16"], out["dx_bf16"] = round_bf16(y), round_bf16(out["dx"])
    return out
