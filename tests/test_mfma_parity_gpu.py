"""GPU parity of the 3x3x3 MFMA convolution family (csrc/conv_mfma.hip: tiled, tiled_n8, direct; csrc/conv_mfma_wgrad.hip: cin1,
wgrad3, wgrad4, wgrad6, bf16, bf16t) with the float64 reference tests/mfma_ref.py.  One test per row of tests/mfma_cases.py and
storage type.  Every test asserts the plan numbers and route names its row declares (ops.conv_mfma_plan / conv_route, with the
alignment of the REAL pointers) before anything is launched, runs the raw entry points mri3d_conv3d_fwd / _fwd_stats / _dgrad /
_wgrad and the *_cat forms on guarded buffers (tests/guard.py), compares EVERY element of every result with the reference, runs a
second time on fresh buffers and requires identical bits, checks the guard bands, the untouched channels of every pitched output
and the workspace behind the bytes the plan asks for, and prints the worst error / bound per output.  Unread channels of a pitched
input hold NaN (a zero weight does not hide a stray read); outputs, statistics partials and workspaces are pre-filled with NaN
payloads; a pass the entry point refuses must return MRI3D_ENOTSUP, a workspace one byte short MRI3D_EWORKSPACE, and both must
write nothing.  A pass whose call leaves the family (a misaligned slice: the generic kernels serve it) is only held to that fact.

The bounds and their derivation: tests/mfma_ref.py; tests/test_mfma_bounds.py keeps them honest on the CPU."""
import pytest
import torch

import mfma_cases as mc
import mfma_run as run
from mri_epilepsy_diagnosis_amd import _lib

pytestmark = pytest.mark.gpu

ENOTSUP, EWORKSPACE = run.ENOTSUP, run.EWORKSPACE


def _bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _all_untouched(o, what):
    o.check(what)
    assert all(o.untouched.values()), "%s: the call wrote %s" % (what, [k for k, v in o.untouched.items() if not v])


@pytest.mark.parametrize("row,dtype", mc.PAIRS, ids=mc.IDS)
def test_mfma_matches_float64_reference(row, dtype):
    real = run.pointer_aligns(row, dtype)
    assert real == {"x": run.align(row, dtype, "x"), "y": run.align(row, dtype, "y")}, real
    pl = run.plans(row, dtype, real)
    wrong = run.declared_mismatches(row, dtype, pl)          # before anything is launched
    assert not wrong, "\n".join(wrong)
    inp = run.make_inputs(row, dtype)
    what = "%s %s" % (row.id, dtype)
    refused = [p for p in row.passes if p in row.refused.get(dtype, ())]
    if refused:
        o = run.run(row, dtype, inp, pl, passes=refused)
        assert all(o.rcs[p] == ENOTSUP for p in refused), (what, o.rcs)
        _all_untouched(o, what + ", refused")
    served = [p for p in row.passes if mc.runs(row, dtype, p)]
    if not served:
        return
    first = run.run(row, dtype, inp, pl)
    assert all(rc == 0 for rc in first.rcs.values()), (what, first.rcs, _lib.lib().mri3d_last_error())
    for p in served:                                          # the plan asserted above is the plan of these pointers
        assert first.aligns[p] == real == {"x": 16, "y": 16}, (what, p, first.aligns[p])
    first.check(what)
    second = run.run(row, dtype, inp, pl)
    second.check(what + ", second run")
    for k, v in first.got.items():
        assert torch.equal(_bits(second.got[k]), _bits(v)), "%s: %s differs between two runs" % (what, k)
    del second
    rep = run.report(run.bounds(row, dtype, inp, pl), first.got)
    for name, ratio, over in rep:
        print("%s %-5s %-28s worst error / bound = %.3g" % (what, name, pl[{"y": "fwd", "stats": "fwd", "dx": "dgrad"}.get(name, "wgrad")]["route"], ratio))
    bad = ["%s: %d elements over the bound, worst error / bound = %.3f" % (name, over, ratio) for name, ratio, over in rep if over]
    assert not bad, what + "\n  " + "\n  ".join(bad)
    short = run.run(row, dtype, inp, pl, short_ws=True)
    assert all(rc == EWORKSPACE for rc in short.rcs.values()), (what, short.rcs)
    _all_untouched(short, what + ", workspace one byte short")
