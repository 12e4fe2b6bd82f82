"""float64 reference and counted error bounds of the marching 3x3x3 convolution (csrc/conv_march.hip): Conv3d(k = 3, stride 1, padding 1)
forward with its fused statistics, and the data gradient.  The reference is F.conv3d on float64 tensors and its autograd data
gradient, evaluated on the STORED values: activations and the incoming gradient rounded to the storage type, the weights rounded to
bf16 where the storage type is bf16 (pack_w_march_kernel rounds them for the matrix unit), the bias in fp32.

Bounds.  u = 2^-24.  Every magnitude comes from the reference, never from the kernel; none is fitted.

  y, dx    (27 Kc + 1) 2u A,  A = |b| + sum |w| |x| over the taps inside the volume (dx: sum |w| |dy|).  An accumulator receives
           27 Kc products, one fused step each, in whatever order, and the epilogue adds the bias: 27 Kc + 1 roundings, each relative
           to a partial sum that A bounds.  SUPPOSITION: the factor 2 allows the matrix unit one ulp (2u) per accumulation step
           instead of the half ulp (u) of round-to-nearest; how the MFMA accumulate rounds inside an instruction (the bf16 K = 32
           form sums 32 products) is not documented for it, so the bound does not rely on round-to-nearest.  bf16 products of
           bf16 factors are exact in fp32.  bf16 storage rounds the result once more: 2^-8 |ref|.  Where A = 0 no term reaches the
           element and the result must be exactly 0 (or exactly the bias).
  stats    the kernel sums a = y - b (the fp32 accumulators) and a^2: per lane in fp32 over the rows and planes of its column
           segment, at most m = 8 rows x seglen planes (v_pk_add_f32 / v_pk_fma_f32: one rounding per value), then the four additions
           of row_sum16 over the 16 voxel lanes, then float64 (8 waves in LDS, the blocks on the host).  With da = 27 Kc 2u A0 the
           bound of one accumulator (A0 = sum |w| |x|, no bias) and g = (m + 4) u / (1 - (m + 4) u):
               |S1 - sum a|   <= sum da + g sum (|a| + da)
               |S2 - sum a^2| <= sum da (2 |a| + da) + g sum (|a| + da)^2
           the first term is what the accumulators are off by, the second the m + 4 roundings of the fp32 chain relative to a
           partial sum of magnitudes; the float64 additions add (8 + blocks) 2^-53 of the same magnitude sums."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
BF16_ULP = 2.0 ** -8
TAPS = 27
F64 = torch.float64


def stored_weights(w, dtype):
    """the weights as the kernel multiplies them, in float64"""
    return (w.to(torch.bfloat16) if dtype == "bf16" else w).double()


def _dgrad(dy, w, shape):
    x = torch.zeros(shape, dtype=F64, requires_grad=True)
    F.conv3d(x, w, None, padding=1).backward(dy)
    return x.grad.detach()


def forward(x, w, b):
    """(y, A, a, A0): y = a + b, A = A0 + |b|, A0 = sum |w| |x|; x (N, Ci, D, H, W), w (Co, Ci, 3, 3, 3), b (Co) or None, float64"""
    a = F.conv3d(x, w, None, padding=1)
    A0 = F.conv3d(x.abs(), w.abs(), None, padding=1)
    if b is None:
        return a, A0, a, A0
    return a + b.view(1, -1, 1, 1, 1), A0 + b.abs().view(1, -1, 1, 1, 1), a, A0


def dgrad(dy, w, shape):
    """(dx, L1): the autograd data gradient and sum |w| |dy|"""
    return _dgrad(dy, w, shape), _dgrad(dy.abs(), w.abs(), shape)


def stored_bound(val, A, kc, dtype):
    b = (TAPS * kc + 1) * 2 * U * A
    return b + BF16_ULP * val.abs() if dtype == "bf16" else b


def stats(a, A0, kc, seglen, blocks):
    """(value (Co, 2), bound (Co, 2)) of [sum a, sum a^2] per channel"""
    s = (0, 2, 3, 4)
    da = TAPS * kc * 2 * U * A0
    k = (8 * seglen + 4) * U
    g = k / (1 - k)
    dbl = (8 + blocks) * 2.0 ** -53
    mag1, mag2 = (a.abs() + da).sum(s), ((a.abs() + da) ** 2).sum(s)
    b1 = da.sum(s) + (g + dbl) * mag1
    b2 = (da * (2 * a.abs() + da)).sum(s) + (g + dbl) * mag2
    return torch.stack((a.sum(s), (a * a).sum(s)), 1), torch.stack((b1, b2), 1)


def compare(want, bound, got):
    """(worst error / bound, elements over the bound) of `got` against the float64 reference, EVERY element; where the bound is 0 the
    value must be exactly the reference's; a NaN counts as infinitely far"""
    got = got.double().reshape(want.shape)
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return float(ratio.max()), int((ratio > 1).sum())
