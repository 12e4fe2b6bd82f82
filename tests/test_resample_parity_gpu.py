"""GPU parity of ops.max_pool3d, ops.max_pool3d_skip and ops.upsample3d (csrc/resample.hip) with the float64 reference
tests/resample_ref.py: one test per row of tests/resample_cases.py (PARITY_POOL, PARITY_UP: the earlier rows and the rows that exist
for one corner of a launch plan) and storage type.  Every test asserts the kernel names and plan numbers its row declares
(ops.pool_plan / ops.upsample_plan with the real tensors' alignments) before anything is launched, runs forward and backward through
the public API, compares EVERY element of y and dx with the reference, runs a second time on fresh tensors and requires identical
bits, and checks the guard bands and untouched channels of every pitched tensor.

Bounds.  u = 2^-24; every magnitude comes from the float64 reference, never from the kernel; the factors count the fp32 roundings
on the longest chain of the kernel's expression (each at most u relative to the quantity rounded).  None is fitted.  A bound of 0
means bit equality, compared through an integer view (NaN positions and payloads included).

  pool y, nearest y        0: a copy.
  pool dx                  T terms (the windows whose tap is this voxel, and the addend): T <= 1 -> 0 (the value itself, the addend
                           itself, or exactly 0 for a voxel in no window); else (T - 1) u L1, L1 = sum |term|: T - 1 additions.
  nearest dx               (T - 1) u L1 likewise: the sum of the T fine voxels of a coarse voxel, weights 1.
  trilinear x2 kernels     weights 0.25 / 0.75 / 1 and their products are exact in fp32 (at most 6 significant bits), as is a
                           product of 0.25 with a value.  K u A, A = sum |w_i| |x_i|, with K counted per kernel:
    upsample2x_fwd_march   P = 0.75 fma(0.75, a, 0.25 b) + 0.25 fma(0.75, c, 0.25 d): the inner fma (1), the product 0.75 * (.) and
                           the sum, or one fma where the compiler contracts them (at most 2); the fine plane fma(0.75, P, 0.25 P') (1):
                           K = 4.
    upsample2x_bwd         64 taps accumulated by fma(w, g, acc) with exact w: the first term is rounded by every one: K = 64.
    upsample2x_bwd_march   the row sum r of 4 fmas (4), the plane sum S_f of 4 fmas over the rows (4), then the D taps: the first is
                           an exact product 0.25 S_f, the other three fmas (3): K = 11.
  slab trilinear kernels   the coordinate is fp32: K u A + sum_a c_a u (in_a + 1) G_a, G_a = sum |w_other| |x(i1_a) - x(i0_a)| the
                           magnitude of d y / d coordinate_a.  c_a = 2: the kernel's fmaf(r, o + 0.5, -0.5) rounds once, at most
                           u in_a; ATen's r * (o + 0.5) - 0.5 rounds the product (at most u (in_a + 1/2)) and the difference (u in_a);
                           o + 0.5 and the fraction src - floor(src) are exact.
    upsample_fwd           l0 = 1 - l1 (1 per axis: 3), the products (wd wh) ww (2), 8 fmas that each round the running sum (8):
                           K = 13.  ATen's nested form w_d (w_h (w_w x + ..) + ..) has 3 + 6 roundings on its longest chain.
    tables+upsample_bwd    per axis l0 = 1 - l1 and, where both taps of a fine voxel are this coarse voxel, l0 + l1 (2 per axis: 6),
                           the two products (2), and one fma per term (T): K = 8 + T with L1 = sum |w| |dy| in place of A, and
                           G_a = the same sum with |d w_a / d coordinate| = 1 in place of w_a.
  bf16 storage             adds 2^-8 |ref| (one bf16 ulp, as tests/test_norm_parity_gpu.py) wherever the bound is not 0; the reference
                           is evaluated on the bf16-rounded inputs.

tests/test_resample_bounds.py keeps the bounds honest on the CPU: torch's own fp32 results and an fp32 emulation of the three x2
kernels stay inside them, and five deliberate errors are flagged."""
import pytest
import torch

import resample_cases as rc
import resample_ref as rr
import resample_run as run

U = rr.U
BF16_ULP = 2.0 ** -8
K_FWD_MARCH, K_BWD_TILE, K_BWD_MARCH, K_SLAB_FWD, K_SLAB_BWD, C_COORD = 4, 64, 11, 13, 8, 2


def _coord(row, g):
    return sum(C_COORD * U * (i + 1) * ga for i, ga in zip(row.sp, g))


def bounds(row, dtype, ref, names):
    """{"y" | "dx": (reference, elementwise bound)}, float64; names = {"fwd", "bwd": kernel name} selects the x2 kernels' counts"""
    sums = (ref["dx_t"] - 1).clamp_min(0) * U * ref["dx_l1"] if "dx_t" in ref else None
    if run.is_pool(row) or row.mode == "nearest":
        by, bdx = torch.zeros_like(ref["y"]), sums
    else:
        if names["fwd"].startswith("upsample2x_fwd_march"):
            by = K_FWD_MARCH * U * ref["y_a"]
        else:
            by = K_SLAB_FWD * U * ref["y_a"] + _coord(row, ref["y_g"])
        if names["bwd"].startswith("upsample2x_bwd_march"):
            bdx = K_BWD_MARCH * U * ref["dx_l1"]
        elif names["bwd"].startswith("upsample2x_bwd"):
            bdx = K_BWD_TILE * U * ref["dx_l1"]
        else:
            bdx = (K_SLAB_BWD + ref["dx_t"]) * U * ref["dx_l1"] + _coord(row, ref["dx_g"])
    out = {"y": (ref["y"], by), "dx": (ref["dx"], bdx)}
    if dtype == "bf16":
        out = {k: (r, torch.where(b > 0, b + BF16_ULP * r.abs(), b)) for k, (r, b) in out.items()}
    return out


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def compare(dtype, want, bound, got):
    """(worst error / bound, elements over the bound) of `got` (CPU tensor of the storage type, logical NCDHW) against the float64
    reference.  Where the bound is 0 the bits of `got` must be those of the reference rounded to the storage type."""
    got = got.contiguous()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    same = _bits(got) == _bits(want.to(run.TORCH[dtype]))
    err = (got.double() - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(same, 0.0, torch.inf).double())
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, torch.inf), ratio)
    ratio = torch.where(same, torch.zeros_like(ratio), ratio)       # identical bits are right whatever they are (NaN, inf)
    return float(ratio.max()), int((ratio > 1).sum())


def report(row, dtype, ref, names, got):
    """[(tensor, worst error / bound, elements over)]"""
    return [(k,) + compare(dtype, want, bound, got[k]) for k, (want, bound) in bounds(row, dtype, ref, names).items()]


def to_cpu(t):
    return t.detach().cpu().contiguous()


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row,dtype", rc.PARITY_PAIRS, ids=rc.PARITY_IDS)
def test_resample_matches_float64_reference(row, dtype):
    inp = run.make_inputs(row, dtype)
    res, guards = run.run_row(row, dtype, inp)                 # asserts the declared plan before it launches anything
    got = {k: to_cpu(v) for k, v in res.items()}
    for what, ss in guards:
        ss.assert_outside_intact("%s %s: %s slice" % (row.id, dtype, what))
    res2, guards2 = run.run_row(row, dtype, inp, check_plan=False)
    for k in res:
        assert torch.equal(_bits(to_cpu(res2[k])), _bits(got[k])), "%s %s: %s differs between two runs" % (row.id, dtype, k)
    for what, ss in guards2:
        ss.assert_outside_intact("%s %s: %s slice, second run" % (row.id, dtype, what))
    del res, res2, guards, guards2
    names = {p: v[0] for p, v in run.plans(row, dtype).items()}
    ref = run.reference(row, inp, sensitivity=tuple(not names[p].startswith("upsample2x") for p in ("fwd", "bwd")))
    rep = report(row, dtype, ref, names, got)
    for name, ratio, over in rep:
        print("%s %s %-3s worst error / bound = %.3f%s" % (row.id, dtype, name, ratio, "  (bit equality)" if ratio == 0 else ""))
    bad = ["%s: %d elements over the bound, worst error / bound = %.3f" % (name, over, ratio) for name, ratio, over in rep if over]
    assert not bad, "%s %s\n  " % (row.id, dtype) + "\n  ".join(bad)
