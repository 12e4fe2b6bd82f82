"""Reference for the Monte-Carlo predictive statistics (csrc/mc_stats.hip): the operator's arithmetic restated in torch, in
float64 by default.  The same code runs in float32 to measure what that precision alone costs (the tests' tolerance)."""
import torch


def mc_ref(logits, dtype=torch.float64):
    """logits [T, nvox, C] (any float dtype) -> dict of mean [nvox, C], variance [nvox, C], entropy [nvox], mutual_info [nvox],
    mask [nvox] (uint8, first maximum) and the three sums the state holds: sum_p, sum_p2 [nvox, C], sum_plogp [nvox]."""
    z = logits.to(dtype)
    T = z.shape[0]
    d = z - z.max(dim=2, keepdim=True).values
    e = d.exp()
    S = e.sum(dim=2, keepdim=True)
    logp = d - S.log()                      # from the logits: finite where p underflows to 0
    p = e / S
    sum_p, sum_p2, sum_plogp = p.sum(0), (p * p).sum(0), (p * logp).sum(2).sum(0)
    mean = sum_p / T
    variance = (sum_p2 / T - mean * mean).clamp_min(0)
    safe = torch.where(mean > 0, mean, torch.ones_like(mean))
    entropy = -(mean * safe.log()).sum(1)   # mean == 0 contributes 0 * log 1 = 0
    mutual_info = (entropy + sum_plogp / T).clamp_min(0)
    return {"mean": mean, "variance": variance, "entropy": entropy, "mutual_info": mutual_info,
            "mask": first_argmax(mean), "sum_p": sum_p, "sum_p2": sum_p2, "sum_plogp": sum_plogp}


def first_argmax(x):
    """Index of the first maximal entry along dim 1, as uint8."""
    is_max = x == x.max(dim=1, keepdim=True).values
    return is_max.to(torch.uint8).argmax(dim=1).to(torch.uint8)


def top2_margin(mean):
    """Difference of the two largest entries along dim 1."""
    top = mean.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def ndhwc_rows(t):
    """A logical (N, C, D, H, W) tensor as [N*D*H*W, C] rows in voxel order."""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])
