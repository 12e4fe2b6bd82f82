"""CPU suite: the launch plan of the cross-entropy / focal kernels (csrc/ce_loss.hip) as mri3d_softmax_ce_index_plan_query answers
it.  Every row of tests/ce_cases.py is held to the corner it declares, the table is shown to reach every instantiation and a loop
that goes round in each bucket, and the query and the argument checks are shown to run without a device."""
import ctypes

import pytest
import torch

import ce_cases
from ce_cases import BF, CASES, F32, case_id
from mri_epilepsy_diagnosis_amd import _lib, ops

EINVAL, ENOTSUP, EWORKSPACE = -1, -2, -4


def _plans(c):
    kw = dict(dtype=c.dtype, x_ld=c.pitch, dice_weight=c.dice_weight, ce_weight=c.ce_weight, gamma=c.gamma)
    vox = c.spatial[0] * c.spatial[1] * c.spatial[2]
    return ops.ce_index_plan(2, vox, c.C, pass_=_lib.PASS_FWD, **kw), ops.ce_index_plan(2, vox, c.C, pass_=_lib.PASS_DGRAD, **kw)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_row_sits_in_the_corner_it_declares(c):
    fwd, bwd = _plans(c)
    for p in (fwd, bwd):
        assert (p["bucket"], p["mode"], p["dice"]) == (c.corner["bucket"], c.corner["mode"], c.corner["dice"]), p
        assert p["lanes"] == 256 * p["blocks"] and p["whole_trips"] * p["lanes"] + p["remainder"] == p["items"]
    if c.corner["fwd"] == "partial":
        assert fwd["blocks"] == 1 and fwd["whole_trips"] <= 1 and 0 < fwd["remainder"] < 256, fwd      # 315 voxels: 256 + 59; vox4: 81 items
    else:
        assert fwd["whole_trips"] >= 2 and fwd["remainder"] > 0, fwd
    if c.corner["bwd"] == "partial":
        assert bwd["whole_trips"] == 0 and bwd["remainder"] % 256 != 0, bwd
    else:
        assert bwd["whole_trips"] >= 1 and bwd["remainder"] > 0 and bwd["blocks"] == 2048, bwd
    if c.corner["mode"] == "vox4" and c.spatial == ce_cases.SMALL:
        assert fwd["items"] == 315 // 4 + 3                      # groups and single voxels; sample 1 starts 3 mod 4 into the batch
    if c.group == "bwd_trips":
        vox = c.spatial[0] ** 3
        assert vox % 2 == 1
        # the smallest odd cube whose backward goes round: the next smaller one does not
        side = c.spatial[0] - 2
        small = ops.ce_index_plan(2, side ** 3, c.C, dtype=c.dtype, pass_=_lib.PASS_DGRAD, dice_weight=c.dice_weight, ce_weight=c.ce_weight)
        assert small["whole_trips"] == 0, small


def test_the_table_reaches_every_instantiation_and_a_round_trip_of_every_bucket():
    modes = {2: ("scalar", "vox4"), 4: ("scalar", "rows4"), 8: ("scalar", "rows4"), 16: ("scalar", "rows4"), 32: ("scalar", "rows4")}
    want = {(b, m, d, t) for b, ms in modes.items() for m in ms for d in (0, 1) for t in (F32, BF)}
    got, fwd_round, bwd_round = set(), set(), set()
    for c in CASES:
        fwd, bwd = _plans(c)
        got.add((fwd["bucket"], fwd["mode"], fwd["dice"], c.dtype))
        if fwd["whole_trips"] >= 2:
            fwd_round.add(fwd["bucket"])
        if bwd["whole_trips"] >= 1:
            bwd_round.add(bwd["bucket"])
    assert got == want, want ^ got
    assert fwd_round == bwd_round == {2, 4, 8, 16, 32}
    # every setting of the issue's lists occurs
    assert {c.gamma for c in CASES} == set(ce_cases.GAMMAS) and {c.weights for c in CASES} == set(ce_cases.WEIGHTS)
    assert {c.kind for c in CASES} >= set(ce_cases.KINDS) and {(c.C, c.pitch) for c in ce_cases.group("pitched")} == set(ce_cases.PITCHED)
    assert {c.C for c in ce_cases.group("base")} >= {2, 3, 8, 9, 12, 17, 20, 32}


def test_alignment_decides_the_read_mode():
    assert ops.ce_index_plan(2, 315, 2)["mode"] == "vox4"
    assert ops.ce_index_plan(2, 315, 2, align_logits=8)["mode"] == "scalar"
    assert ops.ce_index_plan(2, 315, 2, align_labels=2)["mode"] == "scalar"
    assert ops.ce_index_plan(2, 315, 2, x_ld=4)["mode"] == "scalar"
    assert ops.ce_index_plan(2, 315, 8)["mode"] == "rows4"
    assert ops.ce_index_plan(2, 315, 8, align_logits=8)["mode"] == "scalar"
    assert ops.ce_index_plan(2, 315, 8, torch.bfloat16, align_logits=8)["mode"] == "rows4"         # four bf16 are 8 bytes
    assert ops.ce_index_plan(2, 315, 8, x_ld=11)["mode"] == "scalar"
    full = ops.ce_index_plan(2, 160 * 192 * 160, 2, torch.bfloat16, dice_weight=1.0)
    assert (full["blocks"], full["whole_trips"], full["items"]) == (1024, 4, 160 * 192 * 160 // 4)
    full = ops.ce_index_plan(2, 160 * 192 * 160, 32, pass_=_lib.PASS_DGRAD)
    assert (full["blocks"], full["whole_trips"], full["remainder"]) == (2048, 9, 160 * 192 * 160 - 9 * 2048 * 256)


def _geom(n=2, vox=315, c=3, x_ld=None, eps=1e-9, dtype=_lib.F32, gamma=0.0, dice_weight=0.0, ce_weight=1.0):
    return _lib.CeIndexGeom(n, vox, c, c if x_ld is None else x_ld, eps, dtype, gamma, dice_weight, ce_weight)


BAD = [("one class", dict(c=1), ENOTSUP), ("33 classes", dict(c=33), ENOTSUP), ("gamma 0.5", dict(gamma=0.5), EINVAL),
       ("gamma -1", dict(gamma=-1.0), EINVAL), ("gamma 8.5", dict(gamma=8.5), EINVAL), ("gamma nan", dict(gamma=float("nan")), EINVAL),
       ("negative dice weight", dict(dice_weight=-1.0), EINVAL), ("negative ce weight", dict(ce_weight=-0.5, dice_weight=1.0), EINVAL),
       ("both weights zero", dict(ce_weight=0.0), EINVAL), ("infinite weight", dict(ce_weight=float("inf")), EINVAL),
       ("pitch below classes", dict(x_ld=2), EINVAL), ("no samples", dict(n=0), EINVAL), ("no voxels", dict(vox=0), EINVAL),
       ("unknown dtype", dict(dtype=5), ENOTSUP)]


@pytest.mark.parametrize("what,kw,code", BAD, ids=[b[0] for b in BAD])
def test_argument_checks_run_before_any_launch_and_without_a_device(what, kw, code):
    """The pointers are host arrays: a launch would fault; every entry point must return its error first."""
    L = _lib.lib()
    g = _geom(**kw)
    buf = (ctypes.c_double * 4096)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    info = _lib.CeIndexPlanInfo()
    assert L.mri3d_softmax_ce_index_plan_query(ctypes.byref(g), _lib.PASS_FWD, 16, 16, ctypes.byref(info)) == code, what
    assert b"softmax_ce_index_plan_query" in L.mri3d_last_error()
    assert L.mri3d_softmax_ce_index_fwd(ctypes.byref(g), P, P, None, P, P, P, 1 << 30, None) == code, what
    assert b"softmax_ce_index_fwd" in L.mri3d_last_error()
    assert L.mri3d_softmax_ce_index_bwd(ctypes.byref(g), P, P, None, P, P, P, None) == code, what
    assert b"softmax_ce_index_bwd" in L.mri3d_last_error()


def test_workspace_and_null_checks_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_double * 4096)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    info = _lib.CeIndexPlanInfo()
    ce, both = _geom(c=32), _geom(c=32, dice_weight=1.0)
    need_ce, need_both = L.mri3d_softmax_ce_index_workspace_bytes(ctypes.byref(ce)), L.mri3d_softmax_ce_index_workspace_bytes(ctypes.byref(both))
    assert need_ce == 2048 * 2 * 8 and need_both == need_ce + 2048 * 32 * 3 * 8           # the CE-only pass keeps no Dice rows
    for g, need in ((ce, need_ce), (both, need_both)):
        assert L.mri3d_softmax_ce_index_fwd(ctypes.byref(g), P, P, None, P, P, P, need - 1, None) == EWORKSPACE
        assert L.mri3d_softmax_ce_index_fwd(ctypes.byref(g), P, P, None, P, P, None, need, None) == EWORKSPACE
        assert L.mri3d_softmax_ce_index_fwd(ctypes.byref(g), None, P, None, P, P, P, need, None) == EINVAL
        assert L.mri3d_softmax_ce_index_bwd(ctypes.byref(g), P, None, None, P, P, P, None) == EINVAL
    assert L.mri3d_softmax_ce_index_workspace_bytes(None) == 0 and L.mri3d_softmax_ce_index_workspace_bytes(ctypes.byref(_geom(c=33))) == 0
    assert L.mri3d_softmax_ce_index_fwd(None, P, P, None, P, P, P, 1 << 30, None) == EINVAL
    assert L.mri3d_softmax_ce_index_plan_query(None, _lib.PASS_FWD, 16, 16, ctypes.byref(info)) == EINVAL
    assert L.mri3d_softmax_ce_index_plan_query(ctypes.byref(ce), _lib.PASS_FWD, 16, 16, None) == EINVAL
    assert L.mri3d_softmax_ce_index_plan_query(ctypes.byref(ce), _lib.PASS_WGRAD, 16, 16, ctypes.byref(info)) == EINVAL
    assert L.mri3d_softmax_ce_index_plan_query(ctypes.byref(ce), _lib.PASS_FWD, 0, 16, ctypes.byref(info)) == EINVAL


def test_struct_layouts_match_the_header(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"Mri3dCeIndexGeom": _lib.CeIndexGeom, "Mri3dCeIndexPlanInfo": _lib.CeIndexPlanInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mri3d.h"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f, _ in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(out[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(out["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)
    assert [f for f, _ in _lib.CeIndexPlanInfo._fields_] == list(ops.CE_PLAN_FIELDS)


def test_python_refusals_name_what_was_passed():
    from mri_epilepsy_diagnosis_amd.segmentation import losses
    lab = torch.zeros(1, 4, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.softmax_ce_index_loss(torch.zeros(1, 3, 4, 4, 4), lab)                            # CPU logits: no fallback
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.softmax_dice_ce_index_loss(torch.zeros(1, 3, 4, 4, 4), lab)
    for gamma in (0.5, -1.0, 9.0):
        with pytest.raises(RuntimeError, match="gamma must be 0 or in"):
            losses.FocalLoss(gamma=gamma)
    with pytest.raises(RuntimeError, match="not both zero"):
        losses.DiceCELoss(dice_weight=0.0, ce_weight=0.0)
    with pytest.raises(ValueError, match="class weights"):
        losses.CrossEntropyLoss(weight=[1.0, -1.0])
    a, b = losses.DiceCELoss(0.5, 2.0, [1.0, 2.0, 0.0], 2.0), losses.DiceCELoss(0.5, 2.0, torch.tensor([1.0, 2.0, 0.0]), 2.0)
    assert a == b and hash(a) == hash(b) and a != losses.DiceCELoss(0.5, 2.0, [1.0, 2.0, 0.5], 2.0) and a != losses.FocalLoss(2.0)
    assert losses.FocalLoss(2.0) == losses.CrossEntropyLoss(gamma=2.0)                      # the same loss by two names
