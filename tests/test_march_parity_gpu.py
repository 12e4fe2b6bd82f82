"""GPU parity of the marching 3x3x3 convolution (csrc/conv_march.hip: mri3d_conv3d_fwd_march / mri3d_conv3d_dgrad_march) with the
float64 reference tests/march_ref.py.  One test per row of tests/march_cases.py and storage type.  Every test asserts the plan
numbers its row declares (ops.conv_march_plan) before anything is launched, runs the raw entry points on guarded buffers
(tests/guard.py), compares EVERY element of every result with the reference, runs a second time on fresh buffers and requires
identical bits, checks the guard bands and the untouched channels of every pitched output, and prints the worst error / bound.
Unread channels of a pitched input hold NaN (a zero weight does not hide a stray read); the statistics partials are pre-filled
with NaN payloads; a pass the plan refuses must return MRI3D_ENOTSUP and write nothing.

The bounds and their derivation: tests/march_ref.py; tests/test_march_bounds.py keeps them honest on the CPU."""
import ctypes

import pytest
import torch

import march_cases as mc
import march_run as run
from mri_epilepsy_diagnosis_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP, EWORKSPACE = run.EINVAL, run.ENOTSUP, run.EWORKSPACE


def _bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _all_untouched(o, what):
    o.check(what)
    assert all(o.untouched.values()), "%s: a refused call wrote %s" % (what, [k for k, v in o.untouched.items() if not v])


@pytest.mark.parametrize("row,dtype", mc.PAIRS, ids=mc.IDS)
def test_march_matches_float64_reference(row, dtype):
    pl = run.plans(row, dtype)
    wrong = run.declared_mismatches(row, dtype, pl)          # before anything is launched
    assert not wrong, "\n".join(wrong)
    inp = run.make_inputs(row, dtype)
    what = "%s %s" % (row.id, dtype)
    refused = [p for p in row.passes if not mc.runs(row, dtype, p)]
    if refused:
        o = run.run(row, dtype, inp, passes=refused, blocks=16)
        assert all(o.rcs[p] == ENOTSUP for p in refused), (what, o.rcs)
        _all_untouched(o, what + ", refused")
    if len(refused) == len(row.passes):
        return
    first = run.run(row, dtype, inp)
    assert all(rc == 0 for rc in first.rcs.values()), (what, first.rcs, _lib.lib().mri3d_last_error())
    first.check(what)
    second = run.run(row, dtype, inp)
    second.check(what + ", second run")
    for k, v in first.got.items():
        assert torch.equal(_bits(second.got[k]), _bits(v)), "%s: %s differs between two runs" % (what, k)
    del second
    rep = run.report(run.bounds(row, dtype, inp, pl), first.got)
    for name, ratio, over in rep:
        print("%s %-5s worst error / bound = %.3g" % (what, name, ratio))
    bad = ["%s: %d elements over the bound, worst error / bound = %.3f" % (name, over, ratio) for name, ratio, over in rep if over]
    assert not bad, what + "\n  " + "\n  ".join(bad)


def _copy(g, **kw):
    h = type(g)()
    ctypes.memmove(ctypes.byref(h), ctypes.byref(g), ctypes.sizeof(g))
    for k, v in kw.items():
        setattr(h, k, v)
    return h


@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_march_refusals_leave_the_outputs_alone(dtype):
    L = _lib.lib()
    row = mc.row("refusals", 16, 16, (4, 9, 17), stats=True)
    inp = run.make_inputs(row, dtype)
    g = run.geom(row, dtype)
    assert all(L.mri3d_conv3d_march_supported(ctypes.byref(g), c) == 1 for c in run.PASSES.values())
    o = run.run(row, dtype, inp)
    assert o.rcs == {"fwd": 0, "dgrad": 0} and not any(o.untouched.values())          # the row itself is served
    half = 4 if dtype == "f32" else 8
    clauses = {
        "stride 2": _copy(g, sd=2, sh=2, sw=2, dout=2, ho=5, wo=9),
        "dilation 2": _copy(g, dd=2, dh=2, dw=2, pd=2, ph=2, pw=2),
        "kernel size 1": _copy(g, kd=1, kh=1, kw=1, pd=0, ph=0, pw=0),
        "x_ld off the pitch granularity": _copy(g, x_ld=g.x_ld + half // 2),
        "y_ld off the pitch granularity": _copy(g, y_ld=g.y_ld + half // 2),
    }
    for what, bad in clauses.items():
        info = _lib.MarchPlanInfo()
        assert all(L.mri3d_conv3d_march_plan_query(ctypes.byref(bad), c, 0, ctypes.byref(info)) == ENOTSUP for c in run.PASSES.values()), what
        o = run.run(row, dtype, inp, g=bad)
        assert o.rcs == {"fwd": ENOTSUP, "dgrad": ENOTSUP}, (what, o.rcs)
        _all_untouched(o, "march %s (%s)" % (what, dtype))
    o = run.run(row, dtype, inp, base_shift=half // 2)                     # the input 8 bytes off the 16-byte alignment
    assert o.rcs == {"fwd": EINVAL, "dgrad": EINVAL}, o.rcs
    _all_untouched(o, "march misaligned input (%s)" % dtype)
    pl = run.plans(row, dtype)
    for p in row.passes:
        o = run.run(row, dtype, inp, passes=[p], ws_bytes=pl[p]["wp_bytes"] - 1)
        assert o.rcs == {p: EWORKSPACE}, (p, o.rcs)
        _all_untouched(o, "march short workspace (%s %s)" % (p, dtype))
    o = run.run(mc.row("bad-split", 32, 16, (4, 9, 17), split=8), dtype, run.make_inputs(mc.row("bad-split", 32, 16, (4, 9, 17)), dtype))
    assert o.rcs == {"fwd": ENOTSUP, "dgrad": ENOTSUP}, o.rcs              # a split that is no multiple of 16
    _all_untouched(o, "march split of 8 (%s)" % dtype)
