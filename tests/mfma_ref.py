"""float64 reference and counted error bounds of the 3x3x3 MFMA convolution family (csrc/conv_mfma.hip: tiled, tiled_n8, direct;
csrc/conv_mfma_wgrad.hip: cin1, wgrad3, wgrad4, wgrad6, bf16, bf16t): Conv3d(k = 3, padding 1, stride 1 | 2 | 3) forward with its
fused statistics, data gradient and weight gradient.  The reference is F.conv3d on float64 tensors and its autograd gradients
(stride 1: tests/march_ref.forward / dgrad, the same operation), evaluated on the STORED values: activations and the incoming
gradient rounded to the storage type; the weights rounded to bf16 where the kernel multiplies bf16 weights — the tiled kernels on
bf16 tensors (pack_w_mfma_bf16_kernel, pack_w_mfma_n8_kernel<bf16_t>); the direct kernel widens its bf16 activations and multiplies
them with the fp32 weights (pack_w_mfma_kernel) —; bias, dw and db in fp32.

Bounds.  u = 2^-24.  Every magnitude comes from the reference, never from the kernel; none is fitted.

  y, dx    march_ref.stored_bound: (27 Kc + 1) 2u A, A = |b| + sum |w| |x| over the taps inside the volume, plus 2^-8 |ref| in bf16
           storage.  An accumulator receives at most 27 Kc products (a strided data gradient fewer), in whatever order, and the
           epilogue adds the bias.  SUPPOSITION (the same as for the marching kernel): the factor 2 allows the matrix unit one ulp
           (2u) per accumulated product instead of the half ulp of round-to-nearest; how the MFMA rounds inside an instruction is not
           documented, so no bound here relies on round-to-nearest.  The direct kernel's split form (a unit's (kd, kh) pairs spread
           over four waves, summed through LDS) adds 3 more additions: (27 Kc + 4) 2u A.
  stats    the tiled STATS epilogue sums a = y - b (the fp32 accumulators) and a^2 per lane over the TH = 8 rows of a tile in fp32
           (conv_mfma_fwd2_kernel: `s1[r] += a; s2[r] += a * a;` — m = 8 additions; the square is one more rounding per step where
           the compiler does not contract it, counted: 16), then the four additions of row_sum16 over the 16 voxel lanes, then
           float64: per wave over the tiles of its workgroup, the four waves, the workgroups on the host.  With
           da = 27 Kc 2u A0 (A0 = sum |w| |x|, no bias), g1 = 12 u / (1 - 12 u), g2 = 20 u / (1 - 20 u):
               |S1 - sum a|   <= sum da + g1 sum (|a| + da)
               |S2 - sum a^2| <= sum da (2 |a| + da) + g2 sum (|a| + da)^2
           (the form of march_ref.stats) plus (tiles per workgroup + 4 + workgroups) 2^-53 of the same magnitude sums.
  dw, db   (chain + 3) 2u L1 + P 2^-53 L1, L1 = sum |x| |dy| over the voxels of the tap (db: sum |dy|).  chain = the number of
           products ONE wave adds into one accumulator element over all tiles of its workgroup (the plan query's `chain`: tiles per
           workgroup x a quarter of a tile's voxels); the 3 are the cross-wave additions of wgrad_combine_store; the P partials are
           summed in double (wgrad_mfma_reduce_kernel).  dw and db are fp32 in both storage types: no bf16 term.  The products of
           bf16 factors are exact in fp32, as are those by the ones that feed db.
  Where the magnitude sum is 0 no term reaches the element: the result must be exactly 0 (or exactly the bias)."""
import torch
import torch.nn.functional as F

import march_ref as mr

U = mr.U
F64 = torch.float64
compare = mr.compare


def stored_weights(w, dtype, kernel):
    """the weights as the kernel multiplies them, in float64"""
    return (w.to(torch.bfloat16) if dtype == "bf16" and kernel in ("tiled", "tiled_n8") else w).double()


def forward(x, w, b, stride=1):
    """(y, A, a, A0) as march_ref.forward, for a stride"""
    if stride == 1:
        return mr.forward(x, w, b)
    a = F.conv3d(x, w, None, stride=stride, padding=1)
    A0 = F.conv3d(x.abs(), w.abs(), None, stride=stride, padding=1)
    if b is None:
        return a, A0, a, A0
    return a + b.view(1, -1, 1, 1, 1), A0 + b.abs().view(1, -1, 1, 1, 1), a, A0


def _dgrad(dy, w, shape, stride):
    x = torch.zeros(shape, dtype=F64, requires_grad=True)
    F.conv3d(x, w, None, stride=stride, padding=1).backward(dy)
    return x.grad.detach()


def dgrad(dy, w, shape, stride=1):
    """(dx, L1): the autograd data gradient and sum |w| |dy|"""
    if stride == 1:
        return mr.dgrad(dy, w, shape)
    return _dgrad(dy, w, shape, stride), _dgrad(dy.abs(), w.abs(), shape, stride)


def _wgrad(x, dy, wshape):
    w = torch.zeros(wshape, dtype=F64, requires_grad=True)
    F.conv3d(x, w, None, padding=1).backward(dy)
    return w.grad.detach()


def wgrad(x, dy, co):
    """(dw, L1w, db, L1b) of the stride-1 convolution: dw[co, ci, tap] = sum_v x[v + tap - 1, ci] dy[v, co], db = sum_v dy"""
    shape = (co, x.shape[1], 3, 3, 3)
    s = (0, 2, 3, 4)
    return _wgrad(x, dy, shape), _wgrad(x.abs(), dy.abs(), shape), dy.sum(s), dy.abs().sum(s)


def stored_bound(val, A, kc, dtype, extra=0):
    """march_ref.stored_bound with `extra` further fp32 additions (the direct kernel's cross-wave sum: 3)"""
    return mr.stored_bound(val, A, kc, dtype) + extra * 2 * U * A


def wgrad_bound(L1, chain, P):
    return (chain + 3) * 2 * U * L1 + P * 2.0 ** -53 * L1


STAT_ROWS = 8          # TH: the rows of a tile a lane sums in fp32


def stats(a, A0, kc, tiles_per_wg, grid):
    """(value (Co, 2), bound (Co, 2)) of [sum a, sum a^2] per channel"""
    s = (0, 2, 3, 4)
    da = mr.TAPS * kc * 2 * U * A0
    k1, k2 = (STAT_ROWS + 4) * U, (2 * STAT_ROWS + 4) * U
    g1, g2 = k1 / (1 - k1), k2 / (1 - k2)
    dbl = (tiles_per_wg + 4 + grid) * 2.0 ** -53
    mag1, mag2 = (a.abs() + da).sum(s), ((a.abs() + da) ** 2).sum(s)
    b1 = da.sum(s) + (g1 + dbl) * mag1
    b2 = (da * (2 * a.abs() + da)).sum(s) + (g2 + dbl) * mag2
    return torch.stack((a.sum(s), (a * a).sum(s)), 1), torch.stack((b1, b2), 1)
