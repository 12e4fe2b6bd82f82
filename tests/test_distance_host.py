"""CPU suite: what csrc/distance.hip decides on the host — workspace sizes, the limits of the transform, the arguments of the
signed map and of the boundary loss — with null pointers and no device: every refusal comes before any launch."""
import ctypes

import pytest

from mri_epilepsy_diagnosis_amd import _lib, ops

EINVAL, ENOTSUP, EWORKSPACE = -1, -2, -4


def L():
    return _lib.lib()


def test_workspace_queries():
    assert L().mri3d_edt_workspace_bytes(2, 160, 192, 160) >= 2 * 4 * 2 * 160 * 192 * 160
    assert L().mri3d_edt_workspace_bytes(1, 1, 1, 1) > 0
    for bad in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0), (1, 2048, 1024, 1024)):
        assert L().mri3d_edt_workspace_bytes(*bad) == 0, bad
    assert L().mri3d_softmax_boundary_workspace_bytes() == 2048 * 2 * 8


def test_plan_query_limits():
    info = _lib.EdtPlanInfo()
    assert L().mri3d_edt_plan(1, 4, 5, 6, None) == EINVAL
    assert L().mri3d_edt_plan(0, 4, 5, 6, ctypes.byref(info)) == EINVAL
    assert L().mri3d_edt_plan(1, 4, 0, 6, ctypes.byref(info)) == EINVAL
    assert L().mri3d_edt_plan(1, 2048, 1024, 1024, ctypes.byref(info)) == ENOTSUP            # 2^31 voxels
    assert L().mri3d_edt_plan(1, 1, 1, 32511, ctypes.byref(info)) == ENOTSUP                # 32511^2 + 2 >= MRI3D_EDT_INF
    assert L().mri3d_edt_plan(1, 1, 1, 32510, ctypes.byref(info)) == 0
    assert 32510 ** 2 + 2 < ops.EDT_INF <= 32511 ** 2 + 2 and ops.EDT_INF == 0x3f000000
    with pytest.raises(RuntimeError):
        ops.edt_plan((1, 1, 1, 32511))


def test_transform_refusals():
    one = ctypes.c_void_p(256)            # never dereferenced: every case below returns before a launch
    ws = L().mri3d_edt_workspace_bytes(1, 4, 5, 6)
    assert L().mri3d_edt_sq_u8(one, 1, 4, 5, 6, -1, 0, one, one, ws - 1, None) == EWORKSPACE
    assert L().mri3d_edt_sq_u8(one, 1, 4, 5, 6, -1, 0, one, None, ws, None) == EWORKSPACE
    assert L().mri3d_edt_sq_u8(None, 1, 4, 5, 6, -1, 0, one, one, ws, None) == EINVAL
    assert L().mri3d_edt_sq_u8(one, 1, 4, 5, 6, -1, 0, None, one, ws, None) == EINVAL
    assert L().mri3d_edt_sq_u8(one, 1, 4, 5, 6, -2, 0, one, one, ws, None) == EINVAL
    assert L().mri3d_edt_sq_u8(one, 1, 4, 5, 6, 256, 0, one, one, ws, None) == EINVAL
    assert L().mri3d_edt_sq_u8(one, 1, 4, 0, 6, -1, 0, one, one, ws, None) == EINVAL
    assert L().mri3d_edt_sq_u8(one, 1, 1, 1, 32511, -1, 0, one, one, 1 << 30, None) == ENOTSUP
    assert L().mri3d_edt_sq_u8(one, 1, 2048, 1024, 1024, -1, 0, one, one, 1 << 40, None) == ENOTSUP
    assert L().mri3d_edt_threshold_u8(one, 1, 4, 5, 6, -1, 0, -1, 0, one, one, ws, None) == EINVAL       # r2 < 0
    assert L().mri3d_edt_threshold_u8(one, 1, 4, 5, 6, -1, 0, ops.EDT_INF, 0, one, one, ws, None) == EINVAL
    assert L().mri3d_edt_threshold_u8(one, 1, 4, 5, 6, -1, 0, 4, 0, one, one, ws - 1, None) == EWORKSPACE
    assert L().mri3d_edt_threshold_u8(one, 1, 1, 32511, 1, -1, 0, 4, 0, one, one, 1 << 30, None) == ENOTSUP
    assert len(L().mri3d_last_error()) > 0


def _ids(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_signed_map_refusals():
    one = ctypes.c_void_p(256)
    ws = L().mri3d_edt_workspace_bytes(2, 4, 5, 6)
    f = L().mri3d_signed_sqdist_u8
    assert f(one, 2, 4, 5, 6, 3, _ids(1), 1, one, one, ws - 1, None) == EWORKSPACE       # (valid up to the workspace)
    assert f(one, 2, 4, 5, 6, 1, _ids(0), 1, one, one, ws, None) == ENOTSUP              # classes outside 2..32
    assert f(one, 2, 4, 5, 6, 33, _ids(0), 1, one, one, ws, None) == ENOTSUP
    assert f(one, 2, 4, 5, 6, 3, _ids(1), 0, one, one, ws, None) == EINVAL               # K outside 1..32
    assert f(one, 2, 4, 5, 6, 3, _ids(*range(33)), 33, one, one, ws, None) == EINVAL
    assert f(one, 2, 4, 5, 6, 3, _ids(0, 3), 2, one, one, ws, None) == EINVAL            # an id >= C
    assert f(one, 2, 4, 5, 6, 3, _ids(-1), 1, one, one, ws, None) == EINVAL
    assert f(one, 2, 4, 5, 6, 3, None, 1, one, one, ws, None) == EINVAL
    assert f(None, 2, 4, 5, 6, 3, _ids(1), 1, one, one, ws, None) == EINVAL
    assert f(one, 2, 1, 32511, 1, 3, _ids(1), 1, one, one, 1 << 30, None) == ENOTSUP
    with pytest.raises(ValueError):
        ops._class_ids("test", 3, (1, 1))
    with pytest.raises(ValueError):
        ops._class_ids("test", 3, ())


def _geom(n=2, vox=100, c=3, x_ld=3, dtype=_lib.F32, ids=(1,)):
    return _lib.BoundaryGeom(n, vox, c, x_ld, dtype, len(ids), (ctypes.c_int32 * 32)(*ids[:32]))


def test_boundary_loss_refusals():
    one = ctypes.c_void_p(256)
    ws = L().mri3d_softmax_boundary_workspace_bytes()
    fwd, bwd = L().mri3d_softmax_boundary_fwd, L().mri3d_softmax_boundary_bwd

    def both(g):
        a = fwd(ctypes.byref(g), one, one, one, one, one, ws, None)
        b = bwd(ctypes.byref(g), one, one, one, one, one, g.c, None)
        assert a == b
        return a
    assert fwd(ctypes.byref(_geom()), one, one, one, one, one, ws - 1, None) == EWORKSPACE      # (valid up to the workspace)
    assert fwd(None, one, one, one, one, one, ws, None) == EINVAL
    assert both(_geom(c=1, x_ld=1, ids=(0,))) == ENOTSUP
    assert both(_geom(c=33, x_ld=33)) == ENOTSUP
    assert both(_geom(dtype=7)) == ENOTSUP
    assert both(_geom(x_ld=2)) == EINVAL
    assert both(_geom(vox=0)) == EINVAL
    assert both(_geom(ids=())) == EINVAL                                                         # K outside 1..32
    g = _geom()
    g.k = 33
    assert both(g) == EINVAL
    assert both(_geom(ids=(3,))) == EINVAL                                                       # an id >= C
    assert both(_geom(ids=(1, 1))) == EINVAL                                                     # an id twice
    assert fwd(ctypes.byref(_geom()), None, one, one, one, one, ws, None) == EINVAL
    assert bwd(ctypes.byref(_geom()), one, one, one, one, one, 2, None) == EINVAL                # gradient pitch < C
    assert bwd(ctypes.byref(_geom()), one, one, one, one, None, 3, None) == EINVAL
