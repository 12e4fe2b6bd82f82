"""CPU suite: the joint-histogram plan query and the argument validation of csrc/register.hip are host decisions (no device is
touched), and the case table of tests/test_register_gpu.py (tests/register_cases.py) has a row on every corner the plan reports."""
import ctypes

import pytest

import register_cases as RC
from mri_epilepsy_diagnosis_amd import _lib, ops


def _plan(shape, k, bins):
    out = (ctypes.c_int32 * 8)()
    rc = _lib.lib().mri3d_joint_hist_plan(shape[0], shape[1], shape[2], k, bins, out)
    return rc, dict(zip(ops.JOINT_HIST_PLAN_FIELDS, out))


def test_plan_of_the_template_grid():
    rc, p = _plan((182, 218, 182), 64, 64)
    # 39 676 rows = 9919 quads on 512 blocks: 20 trips (19 for the blocks past 9919 - 19 * 512); 16 groups of 4 candidates
    assert rc == 0 and p == dict(blocks=512, groups=16, group_candidates=4, rows_per_trip=4, trips=20, lds_bytes=65536, stages=2,
                                 wave_step=64)
    assert ops.joint_hist_plan((182, 218, 182), 64, 64) == p
    rc, p = _plan((23, 28, 23), 24, 32)
    assert rc == 0 and (p["blocks"], p["groups"], p["trips"], p["lds_bytes"]) == (161, 6, 1, 4 * 32 * 32 * 4)
    rc, p = _plan((1, 3, 5), 2, 16)
    assert rc == 0 and (p["blocks"], p["groups"], p["group_candidates"], p["lds_bytes"]) == (1, 1, 2, 2 * 16 * 16 * 4)


def test_plan_and_workspace_queries_validate_their_arguments():
    L = _lib.lib()
    out = (ctypes.c_int32 * 8)()
    assert L.mri3d_joint_hist_plan(4, 4, 4, 1, 16, None) == -1
    for bad in ((0, 4, 4, 1, 16), (4, -1, 4, 1, 16), (4, 4, 4, 0, 16), (4, 4, 4, 65, 16), (4, 4, 4, 1, 1), (4, 4, 4, 1, 65)):
        assert L.mri3d_joint_hist_plan(*bad, out) == -1 and len(L.mri3d_last_error()) > 0, bad
        assert L.mri3d_joint_hist_workspace_bytes(*bad) == 0, bad
    assert L.mri3d_joint_hist_plan(2048, 2048, 512, 1, 16, out) == -2                       # 2^31 voxels
    assert L.mri3d_joint_hist_workspace_bytes(2048, 2048, 512, 1, 16) == 0
    assert L.mri3d_joint_hist_workspace_bytes(182, 218, 182, 64, 64) == 64 * 64 * 64 * 4
    with pytest.raises(RuntimeError):
        ops.joint_hist_plan((4, 4, 4), 0, 16)


def test_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(1 << 20)            # never dereferenced: validation fails first
    assert L.mri3d_quantize_u8(None, None, 8, 0.0, 1.0, 16, p, None) == -1
    assert L.mri3d_quantize_u8(p, None, 8, 0.0, 1.0, 65, ctypes.c_void_p(2 << 20), None) == -1
    assert L.mri3d_quantize_u8(p, None, 8, 0.0, float("inf"), 16, ctypes.c_void_p(2 << 20), None) == -1
    assert L.mri3d_quantize_u8(p, None, 8, 0.0, 1.0, 16, ctypes.c_void_p((1 << 20) + 16), None) == -1       # out inside x
    q, a, h, w = ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20), ctypes.c_void_p(4 << 20), ctypes.c_void_p(5 << 20)
    assert L.mri3d_joint_hist(p, 4, 4, 4, q, 4, 4, 4, a, 65, 0.0, 1.0, 16, h, w, 1 << 20, None) == -1
    assert L.mri3d_joint_hist(p, 4, 4, 4, q, 4, 4, 0, a, 1, 0.0, 1.0, 16, h, w, 1 << 20, None) == -1
    assert L.mri3d_joint_hist(p, 4, 4, 4, q, 2048, 2048, 512, a, 1, 0.0, 1.0, 16, h, w, 1 << 20, None) == -2
    assert L.mri3d_joint_hist(p, 4, 4, 4, None, 4, 4, 4, a, 1, 0.0, 1.0, 16, h, w, 1 << 20, None) == -1
    assert L.mri3d_joint_hist(p, 4, 4, 4, q, 4, 4, 4, a, 1, 0.0, 1.0, 16, h, w, 16 * 16 * 4 - 1, None) == -4          # workspace too small
    assert L.mri3d_joint_hist(p, 4, 4, 4, q, 4, 4, 4, a, 1, 0.0, 1.0, 16, h, h, 1 << 20, None) == -1                  # hist is the workspace
    assert L.mri3d_joint_hist(p, 4, 4, 4, q, 4, 4, 4, a, 1, 0.0, 1.0, 16, ctypes.c_void_p((4 << 20) + 4), w, 1 << 20, None) == -1
    assert L.mri3d_hist_costs(h, 1, 16, 3, 0.0, w, None) == -1
    assert L.mri3d_hist_costs(h, 1, 16, 0, -1.0, w, None) == -1
    assert L.mri3d_hist_costs(h, 0, 16, 0, 0.0, w, None) == -1
    assert L.mri3d_hist_costs(None, 1, 16, 0, 0.0, w, None) == -1
    assert L.mri3d_resample_affine(None, None, None, None, 0, 4, 4, 4, 4, 4, 4, a, 0.0, None) == -1
    assert L.mri3d_resample_affine(p, None, None, None, 0, 4, 4, 4, 4, 4, 4, a, 0.0, None) == -1
    assert L.mri3d_resample_affine(p, q, h, w, 3, 4, 4, 4, 4, 4, 4, a, 0.0, None) == -1
    assert L.mri3d_resample_affine(p, p, None, None, 0, 4, 4, 4, 4, 4, 4, a, 0.0, None) == -1
    assert L.mri3d_resample_affine(p, q, None, None, 0, 4, 4, 4, 4, 4, 4, None, 0.0, None) == -1
    assert L.mri3d_downsample2_mean_f32(p, 4, 4, 4, p, None) == -1
    assert L.mri3d_downsample2_mean_f32(p, 4, 0, 4, q, None) == -1
    assert L.mri3d_downsample2_mean_f32(p, 2048, 2048, 512, q, None) == -2
    assert len(L.mri3d_last_error()) > 0


def test_the_gpu_case_table_has_a_row_on_every_plan_corner():
    seen = set()
    for name, (fshape, _, k, bins, _, _) in RC.GENERAL_CASES.items():
        rc, p = _plan(fshape, k, bins)
        assert rc == 0, name
        seen |= RC.plan_corners(fshape, k, p)
    assert seen == RC.ALL_CORNERS, RC.ALL_CORNERS ^ seen
    assert {c[3] for c in RC.GENERAL_CASES.values()} == {16, 32, 64} and {1, 5, 64} <= {c[2] for c in RC.GENERAL_CASES.values()}


def test_wrappers_refuse_host_tensors():
    import torch
    x = torch.zeros(4, 4, 4)
    for call in (lambda: ops.quantize_bins(x, 0.0, 1.0, 16), lambda: ops.downsample2(x),
                 lambda: ops.joint_histogram(x.to(torch.uint8), x, torch.eye(4)[:3], 0.0, 1.0, 16),
                 lambda: ops.histogram_costs(torch.zeros(1, 4, 4, dtype=torch.int64)),
                 lambda: ops.resample_affine(x, None, torch.eye(4)[:3], (4, 4, 4))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
