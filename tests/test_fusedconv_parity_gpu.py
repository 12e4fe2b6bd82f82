"""GPU parity of the two fused convolution operators with the float64 reference tests/fusedconv_ref.py: mri3d_upconv3d_fwd / _dgrad /
_wgrad (csrc/upconv.hip, behind ops.upsample_conv3d) and mri3d_convpair_wgrad_first (csrc/sepconv.hip, behind ops.conv3d_pair).  One
test per row of tests/fusedconv_cases.py and storage type.  Every test asserts the plan numbers its row declares (ops.upconv_plan /
ops.conv_pair_plan) before anything is launched, runs the raw entry points on guarded buffers (tests/guard.py), compares EVERY
element of every result with the reference, runs a second time on fresh buffers and requires identical bits, checks the guard bands
and the untouched channels of every pitched output, and prints the worst error / bound.  Unread channels of a pitched input hold NaN
(dy, dy2) or 3e4 (x): a read outside the slice that reaches a result shows.

Bounds.  u = 2^-24; every magnitude comes from the float64 reference evaluated on the stored values, never from the kernel; the
factor counts the fp32 roundings on the longest chain of the kernel's expression (each at most u relative to a partial sum that L1 =
sum |term| bounds).  None is fitted.  Where L1 = 0 (no term reaches the element) the result must be exactly 0.

  upconv y       (taps Ci + 1) u A, A = |b| + sum |w| |x|: upconv_fwd_kernel starts from the bias and adds every term by one fma, taps x Ci
                 of them; the + 1 leaves room for the bias where it is the larger addend.
  upconv dx      (taps Co + 3 log2 S) u L1: the lane of a fine voxel chains taps x Co fmas per input channel, then the butterfly over the
                 S^3 lanes of the coarse voxel adds log2(S^3) = 3 log2 S times, whether a step halves the channels or sums single values.
  upconv dw, dbias   (m + 8) u L1: a lane accumulates one fma (dbias: one addition) per voxel it visits, m = lane-loop trips x slab trips
                 (`trips` x `gtrips` of the weight-gradient plan) at most; 6 xor-shuffle steps and the 2 additions over the four waves
                 make the block's partial; the partials are summed in double.
  pair dw1, dbias1   (3 x 8 + m + 8) u L1, L1 = sum |x| |dy2| |w2| (dbias1: sum |dy2| |w2|): at most 3 taps x 8 channels of fmas form
                 da1 of a voxel, then one fma (addition) per voxel the lane visits, m = row trips x W chunks (`gtrips` x `chunks`), the
                 same tree, the partials in double.
  bf16 storage   y and dx are rounded to bf16 on the store: 2^-8 |ref| more.  dw, dbias, dw1 and dbias1 are fp32 in both storage types.

tests/test_fusedconv_bounds.py keeps the bounds honest on the CPU: the reference agrees with torch's float64 operators, an fp32
emulation of every pass in the kernel's summation order stays inside the bounds, and nine deliberate errors leave them."""
import ctypes

import pytest
import torch

import fusedconv_cases as fc
import fusedconv_run as run
from mri_epilepsy_diagnosis_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -1, -2


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _parity(row, dtype, runner):
    wrong = run.declared_mismatches(row, dtype, run.plans(row, dtype))          # before anything is launched
    assert not wrong, "\n".join(wrong)
    inp = run.make_inputs(row, dtype)
    first = runner(row, dtype, inp)
    assert all(rc == 0 for rc in first.rcs), (row.id, dtype, first.rcs, _lib.lib().mri3d_last_error())
    first.check("%s %s" % (row.id, dtype))
    second = runner(row, dtype, inp)
    second.check("%s %s, second run" % (row.id, dtype))
    for k, v in first.got.items():
        if v is not None:
            assert torch.equal(_bits(second.got[k]), _bits(v)), "%s %s: %s differs between two runs" % (row.id, dtype, k)
    del second
    ref = run.reference(row, inp)
    rep = run.report(row, dtype, ref, run.plans(row, dtype), first.got)
    assert {name for name, _, _ in rep} == {k for k, v in first.got.items() if v is not None}
    for name, ratio, over in rep:
        print("%s %s %-6s worst error / bound = %.3f" % (row.id, dtype, name, ratio))
    bad = ["%s: %d elements over the bound, worst error / bound = %.3f" % (name, over, ratio) for name, ratio, over in rep if over]
    assert not bad, "%s %s\n  " % (row.id, dtype) + "\n  ".join(bad)


@pytest.mark.parametrize("row,dtype", fc.UP_PAIRS, ids=fc.UP_IDS)
def test_upconv_matches_float64_reference(row, dtype):
    _parity(row, dtype, run.run_up)


@pytest.mark.parametrize("row,dtype", fc.PAIR_PAIRS, ids=fc.PAIR_IDS)
def test_convpair_matches_float64_reference(row, dtype):
    _parity(row, dtype, run.run_pair)


def _copy(g, **kw):
    h = type(g)()
    ctypes.memmove(ctypes.byref(h), ctypes.byref(g), ctypes.sizeof(g))
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def _all_untouched(o, what):
    o.check(what)
    assert all(o.untouched.values()), "%s: a refused call wrote %s" % (what, [k for k, v in o.untouched.items() if not v])


@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_upconv_refusals_leave_the_outputs_alone(dtype):
    L = _lib.lib()
    row = fc.up("refusals", 8, 1, (3, 1, 1), 4, (2, 2, 3), (1, 0, 0))
    inp = run.make_inputs(row, dtype)
    g = run.up_geom(row, dtype)
    assert L.mri3d_upconv3d_supported(ctypes.byref(g), 4) == 1 and L.mri3d_upconv3d_workspace_bytes(ctypes.byref(g), 4) > 0
    clauses = {
        "scale 3": (g, 3),
        "extent not divisible by the scale": (_copy(g, hi=g.hi + 2, ho=g.ho + 2), 4),
        "x_ld % 4": (_copy(g, x_ld=g.x_ld + 2), 4),
        "stride 2": (_copy(g, sd=2), 4),
        "dilation 2": (_copy(g, dd=2), 4),
        "no (4, 3, 3) instance": (_copy(g, ci=4, co=3, y_ld=3), 4),
        "mis-stated dout": (_copy(g, dout=g.dout - 1), 4),
    }
    for what, (bad, scale) in clauses.items():
        assert L.mri3d_upconv3d_supported(ctypes.byref(bad), scale) == 0, what
        assert L.mri3d_upconv3d_workspace_bytes(ctypes.byref(bad), scale) == 0, what
        info = _lib.FusedConvPlanInfo()
        assert all(L.mri3d_upconv3d_plan_query(ctypes.byref(bad), scale, p, ctypes.byref(info)) == ENOTSUP for p in (0, 1, 2)), what
        o = run.run_up(row, dtype, inp, geom=bad, scale=scale, refused=True)
        assert o.rcs == [ENOTSUP] * 3, (what, o.rcs)
        _all_untouched(o, "upconv %s (%s)" % (what, dtype))
    o = run.run_up(row, dtype, inp, refused=True, base_shift={"x": 1, "dx": 1})      # bases off the four-element alignment
    assert o.rcs == [EINVAL] * 3, o.rcs
    _all_untouched(o, "upconv misaligned base (%s)" % dtype)
    o = run.run_up(row, dtype, inp, refused=True, ws_short=1)
    assert o.rcs == [0, 0, EINVAL], o.rcs
    o.check("upconv short workspace (%s)" % dtype)
    assert o.untouched["dw"] and o.untouched["dbias"] and not o.untouched["y"] and not o.untouched["dx"]


@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_convpair_refusals_leave_the_outputs_alone(dtype):
    L = _lib.lib()
    row = fc.pair("refusals", (8, 9, 5))
    inp = run.make_inputs(row, dtype)
    first, second = run.pair_geoms(row, dtype)
    assert L.mri3d_convpair_supported(ctypes.byref(first), ctypes.byref(second)) == 1
    clauses = {
        "four taps reach a row": (first, _copy(second, kh=4, sh=1, ph=1, ho=second.hi + 2 - 4 + 1)),
        "nine taps": (first, _copy(second, kh=9, sh=3, ph=3, ho=(second.hi + 6 - 9) // 3 + 1)),
        "co != 8": (_copy(first, co=4, y_ld=4), _copy(second, ci=4, x_ld=4)),
        "y_ld % 4": (first, _copy(second, y_ld=10)),
    }
    for what, (a, b) in clauses.items():
        assert L.mri3d_convpair_supported(ctypes.byref(a), ctypes.byref(b)) == 0, what
        assert L.mri3d_convpair_workspace_bytes(ctypes.byref(a), ctypes.byref(b)) == 0, what
        info = _lib.FusedConvPlanInfo()
        assert L.mri3d_convpair_plan_query(ctypes.byref(a), ctypes.byref(b), ctypes.byref(info)) == ENOTSUP, what
        o = run.run_pair(row, dtype, inp, geoms=(a, b))
        assert o.rcs == [ENOTSUP], (what, o.rcs)
        _all_untouched(o, "pair %s (%s)" % (what, dtype))
    o = run.run_pair(row, dtype, inp, base_shift=1)
    assert o.rcs == [EINVAL], o.rcs
    _all_untouched(o, "pair misaligned dy2 (%s)" % dtype)
    o = run.run_pair(row, dtype, inp, ws_short=1)
    assert o.rcs == [EINVAL], o.rcs
    _all_untouched(o, "pair short workspace (%s)" % dtype)
