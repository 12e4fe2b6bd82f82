"""CPU suite of the label path (csrc/labels.hip, ops.remap_labels / softmax_dice_index_loss / confusion_counts,
segmentation/labels.py): the references the GPU suite compares with are themselves checked (tests/labels_ref.py against the current
prepare_batch and against oracle.losses), the C ABI (symbols, the geometry's layout, host-only queries, every validation branch,
all before any launch), the no-fallback errors and the LabelMap constructors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import labels_ref
from mri_epilepsy_diagnosis_amd import _lib, ops
from mri_epilepsy_diagnosis_amd.segmentation import labels as label_maps, routine
from oracle import losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mri3d_label_remap", "mri3d_softmax_dice_index_workspace_bytes", "mri3d_softmax_dice_index_fwd",
         "mri3d_softmax_dice_index_bwd", "mri3d_confusion_workspace_bytes", "mri3d_confusion_counts")
EINVAL, ENOTSUP, EWORKSPACE = -1, -2, -4
P = ctypes.c_void_p
A, B, C_, D = 0x10000, 0x2000000, 0x4000000, 0x6000000      # non-NULL, far apart: validation never dereferences and returns before any launch


# ------------------------------------------------------------------------------------------------ the references
def _edge_batch(dtype):
    """(2, 1, 4, 6, 8) labels: every edge value the dtype can hold, LIST_FCD ids and ids around 1000, in both samples."""
    info = None if dtype.is_floating_point else torch.iinfo(dtype)
    vals = [v for v in labels_ref.EDGE_VALUES if info is None or (v == v and abs(v) != float("inf") and v == int(v) and info.min <= v <= info.max)]
    vals += labels_ref.LIST_FCD + [1, 2, 7, 9, 1001, 2035, 1999]
    g = torch.Generator().manual_seed(3)
    fill = torch.randint(0, 2100 if info is None or info.max > 2100 else 256, (2 * 4 * 6 * 8,), generator=g).double()
    fill[:len(vals)] = torch.tensor(vals, dtype=torch.float64)
    fill[192:192 + len(vals)] = torch.tensor(vals, dtype=torch.float64)      # the same values in the second sample
    return fill.to(dtype).reshape(2, 1, 4, 6, 8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16, torch.int32], ids=["float32", "int16", "int32"])
def test_remap_reference_is_the_current_prepare_batch(dtype):
    raw = _edge_batch(dtype)
    want = labels_ref.binarise_ref(raw.numpy())
    batch = {routine.MRI: {routine.DATA: torch.zeros(2, 1, 4, 6, 8)}, routine.LABEL: {routine.DATA: raw.clone()}}
    _, got = routine.prepare_batch(batch, "cpu")
    assert got.dtype == dtype and np.array_equal(got.numpy(), want)
    # the first-sample quirk shows: a LIST_FCD id is 1 in sample 0 and 0 in sample 1
    where = ((raw[0] == 8) & (raw[1] == 8)).nonzero()[0]
    assert float(got[0][tuple(where)]) == 1 and float(got[1][tuple(where)]) == 0


def test_remap_reference_rule():
    lut = np.arange(10, dtype=np.uint8) + 100
    v = np.array([np.nan, np.inf, -np.inf, -1, -0.0, 0.5, 9, 9.5, 10, 10.5, 3], dtype=np.float32)
    assert labels_ref.remap_ref(v, lut, 7, 5).tolist() == [5, 7, 5, 5, 100, 5, 109, 5, 7, 7, 103]
    assert labels_ref.remap_ref(np.array([-3, 0, 9, 10, 30000], np.int16), lut, 7, 5, np.float32).tolist() == [5, 100, 109, 7, 7]
    assert labels_ref.remap_ref(np.array([0, 9, 10, 255], np.uint8), lut, 7, 5).tolist() == [100, 109, 7, 7]


def test_dice_reference_is_the_oracle_loss_on_a_one_hot():
    g = torch.Generator().manual_seed(0)
    for C in (2, 5, 9, 32):
        z = (3.0 * torch.randn(2, C, 3, 4, 5, generator=g)).double()
        lab = torch.randint(0, C, (2, 3, 4, 5), generator=g).to(torch.uint8)
        want = losses.softmax_dice_loss(z, labels_ref.one_hot(lab, C))
        assert abs(labels_ref.dice_index_loss(z, lab).item() - want.item()) <= 1e-12
    lab[0, 0, 0, :3] = torch.tensor([C, 200, 255], dtype=torch.uint8)      # labels that are no class: zero rows
    oh = labels_ref.one_hot(lab, C)
    assert oh[0, :, 0, 0, :3].abs().sum() == 0 and oh.sum() == lab.numel() - 3
    assert abs(labels_ref.dice_index_loss(z, lab).item() - losses.softmax_dice_loss(z, oh).item()) <= 1e-12


def test_confusion_reference():
    conf, outside = labels_ref.confusion_ref([0, 1, 1, 2, 7], [0, 1, 2, 2, 1], 3)
    assert conf.tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 1]] and outside == 1
    dice, iou = labels_ref.class_scores_ref(np.array([[3, 1, 0], [0, 2, 0], [0, 0, 0]]))
    assert dice[:2].tolist() == [6 / 7, 4 / 5] and iou[:2].tolist() == [3 / 4, 2 / 3] and np.isnan(dice[2]) and np.isnan(iou[2])
    d2, i2 = ops.class_scores_from_confusion(np.array([[3, 1, 0], [0, 2, 0], [0, 0, 0]]))
    assert d2[:2].tolist() == dice[:2].tolist() and np.isnan(d2[2]) and np.isnan(i2[2])
    assert np.allclose(i2[:2], iou[:2], rtol=2.0 ** -23, atol=0)          # the reference's IoU divides float32 counts


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mri3d.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), "%s is not declared in mri3d.h" % n
        assert re.search(r"\bT %s$" % n, nm, flags=re.M), "%s is not exported" % n
        assert n in _lib.SIGNATURES
    for i, name in enumerate(("U8", "I16", "I32", "F32")):
        assert re.search(r"MRI3D_LABEL_%s\s*=\s*%d\b" % (name, i), header) and getattr(_lib, "LABEL_" + name) == i


def test_geometry_layout_matches_header(tmp_path):
    cls, cname = _lib.DiceIndexGeom, "Mri3dDiceIndexGeom"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mri3d.h"', 'int main(void){',
             'printf("size %%zu\\n", sizeof(%s));' % cname]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f, _ in cls._fields_]
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    assert [f for f, _ in cls._fields_] == ["n", "vox", "c", "x_ld", "eps", "dtype"]
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def _geom(n=2, vox=315, c=5, x_ld=None, eps=1e-9, dtype=_lib.F32):
    return _lib.DiceIndexGeom(n, vox, c, c if x_ld is None else x_ld, eps, dtype)


def test_workspace_queries_are_host_only():
    L = _lib.lib()
    q = L.mri3d_softmax_dice_index_workspace_bytes
    assert q(None) == 0
    for c in range(2, 33):
        assert q(ctypes.byref(_geom(c=c))) >= 2 * c * 3 * 8
        assert q(ctypes.byref(_geom(c=c, vox=160 * 192 * 160))) == q(ctypes.byref(_geom(c=c)))       # fixed by the block cap
    assert q(ctypes.byref(_geom(n=5000))) > q(ctypes.byref(_geom(n=2)))                            # one block per sample at least
    for bad in (1, 0, -1, 33):
        assert q(ctypes.byref(_geom(c=bad))) == 0 and L.mri3d_confusion_workspace_bytes(bad) == 0
    for c in range(2, 33):
        assert L.mri3d_confusion_workspace_bytes(c) >= (c * c + 1) * 8


def _remap(inp=A, in_dtype=_lib.LABEL_F32, out=B, out_dtype=_lib.LABEL_U8, n=1000, lut=C_, lut_len=1000, above=1, other=0):
    return _lib.lib().mri3d_label_remap(P(inp), in_dtype, P(out), out_dtype, n, P(lut), lut_len, above, other, None)


REMAP_BRANCHES = [
    ("NULL in", dict(inp=None), EINVAL),
    ("NULL out", dict(out=None), EINVAL),
    ("NULL lut", dict(lut=None), EINVAL),
    ("n = 0", dict(n=0), EINVAL),
    ("n < 0", dict(n=-4), EINVAL),
    ("unknown input dtype", dict(in_dtype=4), ENOTSUP),
    ("negative input dtype", dict(in_dtype=-1), ENOTSUP),
    ("int16 output", dict(out_dtype=_lib.LABEL_I16), ENOTSUP),
    ("unknown output dtype", dict(out_dtype=7), ENOTSUP),
    ("lut_len = 0", dict(lut_len=0), EINVAL),
    ("lut_len = 65537", dict(lut_len=65537), EINVAL),
    ("above = 256", dict(above=256), EINVAL),
    ("other = -1", dict(other=-1), EINVAL),
    ("float32 out aliasing an int32 in", dict(in_dtype=_lib.LABEL_I32, out=A, out_dtype=_lib.LABEL_F32), EINVAL),
    ("float32 out aliasing an int16 in", dict(in_dtype=_lib.LABEL_I16, out=A, out_dtype=_lib.LABEL_F32), EINVAL),
    ("uint8 out aliasing a float32 in", dict(out=A), EINVAL),
    ("out inside in", dict(out=A + 16, out_dtype=_lib.LABEL_F32), EINVAL),
    ("out over the table", dict(out=C_ + 8), EINVAL),
    ("float32 in off its element", dict(inp=A + 2), EINVAL),
    ("float32 out off its element", dict(out=B + 1, out_dtype=_lib.LABEL_F32), EINVAL),
]


@pytest.mark.parametrize("what,kw,code", REMAP_BRANCHES, ids=[b[0] for b in REMAP_BRANCHES])
def test_remap_validation(what, kw, code):
    assert _remap(**kw) == code, what
    msg = _lib.lib().mri3d_last_error()
    assert msg and b"label_remap" in msg, msg


def _fwd(g=None, logits=A, labels=B, loss=C_, stats=C_ + 64, ws=D, ws_bytes=None):
    L = _lib.lib()
    g = _geom() if g is None else g
    if ws_bytes is None or ws_bytes == "one short":
        ws_bytes = L.mri3d_softmax_dice_index_workspace_bytes(ctypes.byref(g)) - (ws_bytes is not None)
    return L.mri3d_softmax_dice_index_fwd(ctypes.byref(g), P(logits), P(labels), P(loss), P(stats), P(ws), ws_bytes, None)


def _bwd(g=None, logits=A, labels=B, stats=C_, dloss=C_ + 4096, dlogits=D):
    g = _geom() if g is None else g
    return _lib.lib().mri3d_softmax_dice_index_bwd(ctypes.byref(g), P(logits), P(labels), P(stats), P(dloss), P(dlogits), None)


GEOM_BRANCHES = [
    ("n = 0", dict(n=0), EINVAL),
    ("vox = 0", dict(vox=0), EINVAL),
    ("unknown dtype", dict(dtype=7), ENOTSUP),
    ("C = 1", dict(c=1), ENOTSUP),
    ("C = 0", dict(c=0), ENOTSUP),
    ("C = 33", dict(c=33), ENOTSUP),
    ("x_ld < C", dict(c=5, x_ld=4), EINVAL),
]
FWD_BRANCHES = [(w, dict(g=_geom(**kw), ws_bytes=1 << 22), code) for w, kw, code in GEOM_BRANCHES] + [
    ("NULL logits", dict(logits=None), EINVAL),
    ("NULL labels", dict(labels=None), EINVAL),
    ("NULL loss", dict(loss=None), EINVAL),
    ("NULL stats", dict(stats=None), EINVAL),
    ("NULL workspace", dict(ws=None), EWORKSPACE),
    ("workspace one byte short", dict(ws_bytes="one short"), EWORKSPACE),
    ("workspace off 8 bytes", dict(ws=D + 4), EWORKSPACE),
]
BWD_BRANCHES = [(w, dict(g=_geom(**kw)), code) for w, kw, code in GEOM_BRANCHES] + [
    ("NULL logits", dict(logits=None), EINVAL),
    ("NULL labels", dict(labels=None), EINVAL),
    ("NULL stats", dict(stats=None), EINVAL),
    ("NULL dloss", dict(dloss=None), EINVAL),
    ("NULL dlogits", dict(dlogits=None), EINVAL),
]


@pytest.mark.parametrize("what,kw,code", FWD_BRANCHES, ids=[b[0] for b in FWD_BRANCHES])
def test_dice_index_fwd_validation(what, kw, code):
    assert _fwd(**kw) == code, what
    msg = _lib.lib().mri3d_last_error()
    assert msg and b"softmax_dice_index_fwd" in msg, msg


def test_dice_float_fwd_refuses_a_workspace_off_8_bytes():
    """The float-target forward goes through the same workspace check: its partial sums are doubles too."""
    L = _lib.lib()
    g = _lib.DiceGeom(2, 315, 2, 1, 2, 1, 1e-9, _lib.F32)
    need = L.mri3d_softmax_dice_workspace_bytes(ctypes.byref(g))
    assert L.mri3d_softmax_dice_fwd(ctypes.byref(g), P(A), P(B), P(C_), P(C_ + 64), P(D + 4), need + 8, None) == EWORKSPACE
    msg = L.mri3d_last_error()
    assert msg and b"softmax_dice_fwd" in msg and b"8-byte aligned" in msg, msg


@pytest.mark.parametrize("what,kw,code", BWD_BRANCHES, ids=[b[0] for b in BWD_BRANCHES])
def test_dice_index_bwd_validation(what, kw, code):
    assert _bwd(**kw) == code, what
    msg = _lib.lib().mri3d_last_error()
    assert msg and b"softmax_dice_index_bwd" in msg, msg


def test_null_geometry():
    L = _lib.lib()
    assert L.mri3d_softmax_dice_index_fwd(None, P(A), P(B), P(C_), P(C_), P(D), 1 << 22, None) == EINVAL
    assert L.mri3d_softmax_dice_index_bwd(None, P(A), P(B), P(C_), P(C_), P(D), None) == EINVAL


def _confusion(pred=A, gt=B, nvox=1000, c=5, counts=C_, ws=D, ws_bytes=None):
    L = _lib.lib()
    if ws_bytes is None or ws_bytes == "one short":
        ws_bytes = L.mri3d_confusion_workspace_bytes(c) - (ws_bytes is not None)
    return L.mri3d_confusion_counts(P(pred), P(gt), nvox, c, P(counts), P(ws), ws_bytes, None)


CONFUSION_BRANCHES = [
    ("NULL pred", dict(pred=None), EINVAL),
    ("NULL gt", dict(gt=None), EINVAL),
    ("NULL counts", dict(counts=None), EINVAL),
    ("counts off 8 bytes", dict(counts=C_ + 4), EINVAL),
    ("nvox = 0", dict(nvox=0), EINVAL),
    ("C = 1", dict(c=1, ws_bytes=1 << 22), ENOTSUP),
    ("C = 33", dict(c=33, ws_bytes=1 << 22), ENOTSUP),
    ("NULL workspace", dict(ws=None), EWORKSPACE),
    ("workspace one byte short", dict(ws_bytes="one short"), EWORKSPACE),
    ("workspace one byte short, C = 2", dict(c=2, ws_bytes="one short"), EWORKSPACE),
]


@pytest.mark.parametrize("what,kw,code", CONFUSION_BRANCHES, ids=[b[0] for b in CONFUSION_BRANCHES])
def test_confusion_validation(what, kw, code):
    assert _confusion(**kw) == code, what
    msg = _lib.lib().mri3d_last_error()
    assert msg and b"confusion_counts" in msg, msg


# ------------------------------------------------------------------------------------------------ the Python layers
def test_cpu_tensors_have_no_fallback():
    lut = torch.zeros(10, dtype=torch.uint8)
    lab = torch.zeros(1, 1, 4, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        ops.remap_labels(torch.zeros(8), lut)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        ops.softmax_dice_index_loss(torch.zeros(1, 3, 4, 4, 4), lab)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        ops.confusion_counts(lab, lab, 3)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        label_maps.LabelMap.from_ids([3, 4])(torch.zeros(1, 1, 4, 4, 4))
    batch = {routine.MRI: {routine.DATA: torch.zeros(1, 1, 4, 4, 4)}, routine.LABEL: {routine.DATA: torch.zeros(1, 1, 4, 4, 4)}}
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        label_maps.prepare_batch_index(batch, "cpu", label_maps.LabelMap.binary_fcd())


def test_label_map_constructors():
    first, plain = labels_ref.fcd_luts()
    b = label_maps.LabelMap.binary_fcd()
    assert (b.above, b.other, b.classes) == (1, 0, 2)
    assert b.lut.dtype == np.uint8 and np.array_equal(b.lut, plain) and np.array_equal(b.first_lut, first)
    assert plain.sum() == 1 and plain[1] == 1 and sorted(np.nonzero(first)[0].tolist()) == sorted(routine.LIST_FCD + [1])
    m = label_maps.LabelMap.from_ids([17, 53, 1006, 2035])
    assert m.lut.shape == (2036,) and m.first_lut is None and (m.above, m.other, m.classes) == (0, 0, 5)
    assert [int(m.lut[i]) for i in (17, 53, 1006, 2035)] == [1, 2, 3, 4] and int(m.lut.sum()) == 10
    g = label_maps.LabelMap.from_groups({1: [17, 53], 3: [1006], 2: [2035, 4]})
    assert g.lut.shape == (2036,) and g.classes == 4
    assert [int(g.lut[i]) for i in (4, 17, 53, 1006, 2035)] == [2, 1, 1, 3, 2] and int((g.lut != 0).sum()) == 5
    assert label_maps.LabelMap(np.array([0, 1, 2]), above=9, other=4).classes == 10
    for bad in (lambda: label_maps.LabelMap.from_ids([]), lambda: label_maps.LabelMap.from_ids([5, 5]),
                lambda: label_maps.LabelMap.from_ids([-1]), lambda: label_maps.LabelMap.from_ids([65536]),
                lambda: label_maps.LabelMap.from_groups({0: [3]}), lambda: label_maps.LabelMap.from_groups({256: [3]}),
                lambda: label_maps.LabelMap(np.zeros(0)), lambda: label_maps.LabelMap(np.zeros(65537)),
                lambda: label_maps.LabelMap(np.zeros(4), above=256)):
        with pytest.raises(ValueError):
            bad()


def test_routine_entry_points_take_a_prepare_hook():
    import inspect
    for fn in (routine.run_epoch, routine.train, routine.validate_dsc_asd, routine.validate_dsc_asd_mc):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "prepare" and params[-1].default is None, fn.__name__
    assert list(inspect.signature(routine.validate_classes).parameters) == ["model", "loader", "label_map", "prepare"]
