"""CPU suite of the connected-components family: the plan query and the entry points' validation (host only), the reference
(tests/components_ref.py) against a brute-force flood fill, the case table (tests/components_cases.py) against the plan's corners,
and the GPU suite's comparison against planted mistakes."""
import ctypes

import numpy as np
import pytest

from mri_epilepsy_diagnosis_amd import _lib, ops

import components_cases as cc
import components_ref as ref

FAKE = ctypes.c_void_p(4096)      # a non-null pointer for arguments the host validation never dereferences
FIELDS = ["td", "th", "tw", "tiles_d", "tiles_h", "tiles_w", "grid_local", "grid_merge", "grid_roots", "grid_scan", "grid_rank",
          "grid_relabel", "scan_blocks", "offsets", "lds_bytes", "ws_bytes"]


def test_plan_query_rows_and_errors():
    assert [f for f, _ in _lib.ComponentsPlanInfo._fields_] == FIELDS == list(ops.COMPONENTS_PLAN_FIELDS)
    L = _lib.lib()
    # a full-size volume: 20 x 24 x 5 tiles of 8 x 8 x 32; 4 915 200 voxels in blocks of 2048; streaming grids capped at 2048
    assert ops.components_plan((160, 192, 160), 26) == dict(
        td=8, th=8, tw=32, tiles_d=20, tiles_h=24, tiles_w=5, grid_local=2400, grid_merge=2048, grid_roots=2400, grid_scan=1,
        grid_rank=2400, grid_relabel=2048, scan_blocks=2400, offsets=13, lds_bytes=2048 * 4 + 2048, ws_bytes=4915200 * 4 + 9728)
    # below a tile in every axis: one tile, one block everywhere; 420 bytes of parents and 4 of counts, each padded to 256
    assert ops.components_plan((3, 5, 7), 6) == dict(
        td=8, th=8, tw=32, tiles_d=1, tiles_h=1, tiles_w=1, grid_local=1, grid_merge=1, grid_roots=1, grid_scan=1, grid_rank=1,
        grid_relabel=1, scan_blocks=1, offsets=3, lds_bytes=10240, ws_bytes=512 + 256)
    # a 2-D map: 2 x 3 tiles, 630 voxels in 3 blocks of 256 threads, one block of 2048
    want = dict(td=8, th=8, tw=32, tiles_d=1, tiles_h=2, tiles_w=3, grid_local=6, grid_merge=3, grid_roots=1, grid_scan=1,
                grid_rank=1, grid_relabel=3, scan_blocks=1, offsets=9, lds_bytes=10240, ws_bytes=2560 + 256)
    assert ops.components_plan((1, 9, 70), 18) == want == ops.components_plan((9, 70), 2)
    assert ops.components_plan((1, 9, 70), 18)["ws_bytes"] == L.mri3d_components_workspace_bytes(1, 9, 70)
    info = _lib.ComponentsPlanInfo()
    assert L.mri3d_components_plan_query(3, 5, 7, 6, None) == -1
    assert L.mri3d_components_plan_query(3, 5, 7, 7, ctypes.byref(info)) == -1
    assert L.mri3d_components_plan_query(0, 5, 7, 6, ctypes.byref(info)) == -1
    assert L.mri3d_components_plan_query(2048, 1024, 1024, 6, ctypes.byref(info)) == -2          # 2^31 voxels
    assert L.mri3d_components_plan_query(2047, 1024, 1024, 6, ctypes.byref(info)) == 0 and info.scan_blocks == 2047 * 512
    assert L.mri3d_components_workspace_bytes(2048, 1024, 1024) == 0 and L.mri3d_components_workspace_bytes(0, 1, 1) == 0
    with pytest.raises(ValueError, match="connectivity"):
        ops.components_plan((3, 5, 7), 7)


def test_struct_layout_matches_header(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mri3d.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(Mri3dComponentsPlanInfo));']
    lines += ['printf("%s %%zu\\n", offsetof(Mri3dComponentsPlanInfo, %s));' % (f, f) for f in FIELDS] + ["return 0;}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_lib.ComponentsPlanInfo)
    for f in FIELDS:
        assert int(out[f]) == getattr(_lib.ComponentsPlanInfo, f).offset, f


def test_entry_points_validate_on_the_host():
    L = _lib.lib()
    EINVAL, ENOTSUP, EWORKSPACE = -1, -2, -4
    big = 1 << 40
    label = L.mri3d_components_label
    assert label(None, 3, 5, 7, 6, 0, FAKE, FAKE, FAKE, big, None) == EINVAL
    assert label(FAKE, 3, 5, 7, 6, 0, None, FAKE, FAKE, big, None) == EINVAL
    assert label(FAKE, 3, 5, 7, 6, 0, FAKE, None, FAKE, big, None) == EINVAL
    assert label(FAKE, 3, 0, 7, 6, 0, FAKE, FAKE, FAKE, big, None) == EINVAL
    assert label(FAKE, 3, 5, 7, 7, 0, FAKE, FAKE, FAKE, big, None) == EINVAL and b"connectivity 7" in L.mri3d_last_error()
    assert label(FAKE, 2048, 1024, 1024, 6, 0, FAKE, FAKE, FAKE, big, None) == ENOTSUP
    need = L.mri3d_components_workspace_bytes(3, 5, 7)
    assert label(FAKE, 3, 5, 7, 6, 0, FAKE, FAKE, FAKE, need - 1, None) == EWORKSPACE
    assert label(FAKE, 3, 5, 7, 6, 0, FAKE, FAKE, None, need, None) == EWORKSPACE
    stats = L.mri3d_components_stats
    assert stats(None, 3, 5, 7, 4, None, None, FAKE, None, None, 0, None, None) == EINVAL
    assert stats(FAKE, 3, 5, 7, 4, None, None, None, None, None, 0, None, None) == EINVAL
    assert stats(FAKE, 3, 5, 7, 0, None, None, FAKE, None, None, 0, None, None) == EINVAL                 # no rows
    assert stats(FAKE, 3, 5, 7, 4, None, FAKE, FAKE, None, None, 0, None, None) == EINVAL                 # a score without a peak
    assert stats(FAKE, 3, 5, 7, 4, None, None, FAKE, None, FAKE, 0, FAKE, None) == EINVAL                 # other labels, no rows
    assert stats(FAKE, 3, 5, 7, 4, None, None, FAKE, None, None, 2, FAKE, None) == EINVAL                 # a hit table, no labels
    assert stats(FAKE, 2048, 1024, 1024, 4, None, None, FAKE, None, None, 0, None, None) == ENOTSUP
    select = L.mri3d_components_select
    assert select(None, 10, FAKE, 3, FAKE, None) == EINVAL and select(FAKE, 10, None, 3, FAKE, None) == EINVAL
    assert select(FAKE, 10, FAKE, 3, None, None) == EINVAL and select(FAKE, 0, FAKE, 3, FAKE, None) == EINVAL
    assert select(FAKE, 10, FAKE, 0, FAKE, None) == EINVAL


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from mri_epilepsy_diagnosis_amd.segmentation import components
    mask = torch.zeros(3, 4, 5, dtype=torch.uint8)
    lab = torch.zeros(3, 4, 5, dtype=torch.int32)
    for call in (lambda: ops.label_components(mask), lambda: ops.component_stats(lab, 3),
                 lambda: ops.select_components(lab, torch.zeros(2, dtype=torch.uint8)), lambda: components.components(mask),
                 lambda: components.remove_small(mask, 3), lambda: components.keep_largest(mask), lambda: components.lesion_scores(mask, mask),
                 lambda: components.rank_clusters(mask, mask.float())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


@pytest.mark.parametrize("connectivity", cc.CONNECTIVITIES)
def test_reference_against_flood_fill(connectivity):
    rng = np.random.default_rng(connectivity)
    shapes = [(6, 6, 6), (1, 5, 6), (4, 1, 6), (5, 6, 1), (2, 3, 4), (1, 1, 1)]
    for shape in shapes:
        for p in (0.25, 0.5, 0.8):
            m = (rng.random(shape) < p).astype(np.uint8)
            ref.assert_same_labelling(*ref.label(m, connectivity), *ref.flood_label(m, connectivity), what="binary %s" % (shape,))
            v = m * rng.integers(1, 4, shape).astype(np.uint8)
            ref.assert_same_labelling(*ref.label(v, connectivity, True), *ref.flood_label(v, connectivity, True), what="by value %s" % (shape,))
            ref.assert_same_labelling(*ref.label(v, connectivity), *ref.flood_label(m, connectivity), what="values as a mask %s" % (shape,))


def test_reference_statistics_by_hand():
    m = np.zeros((2, 3, 4), dtype=np.uint8)
    m[0, 0, 0:2] = 1          # id 1: two voxels
    m[1, 2, 3] = 1            # id 2: one voxel
    other = np.zeros_like(m)
    other[0, 0, 1] = other[1, 2, 3] = other[1, 0, 0] = 1
    score = np.arange(24, dtype=np.float32).reshape(2, 3, 4) - 5
    lab, k = ref.label(m, 6)
    assert k == 2
    table, peak = ref.stats(lab, 3, other, score)
    assert table.tolist() == [[2, 1, 0, 0, 0, 0, 0, 1], [1, 1, 1, 1, 2, 2, 3, 3], [0, 0, 2, -1, 3, -1, 4, -1]]
    assert peak.tolist() == [-4.0, 18.0, -np.inf]
    olab, ok = ref.label(other, 6)
    assert ok == 3 and ref.hit(lab, olab, 3).tolist() == [1, 0, 1]
    s = ref.lesion_scores(m, other, 6)
    assert (s["n_lesions"], s["n_clusters"], s["lesions_detected"], s["clusters_true"], s["clusters_false"]) == (3, 2, 2, 2, 0)
    assert s["sensitivity"] == 2 / 3 and s["precision"] == 1.0
    assert np.isnan(ref.lesion_scores(np.zeros_like(m), np.zeros_like(m), 6)["sensitivity"])


def test_case_table_reaches_every_plan_corner():
    cases = cc.build()
    td, th, tw = T = cc.tile()
    assert len({c.name for c in cases}) == len(cases)
    shapes = [ref.as3d(c.mask).shape for c in cases]
    for axis in range(3):
        ext = {s[axis] for s in shapes}
        assert any(e < T[axis] for e in ext) and T[axis] in ext and T[axis] + 1 in ext and any(e > 2 * T[axis] for e in ext), axis
    plans = [ops.components_plan(s, 26) for s in shapes]
    assert {min(p["scan_blocks"], 2) for p in plans} == {1, 2}                  # one and several scan blocks
    assert {min(p["grid_local"], 2) for p in plans} == {1, 2} and {min(p["grid_merge"], 2) for p in plans} == {1, 2}
    assert any(p["tiles_d"] > 1 and p["tiles_h"] > 1 and p["tiles_w"] > 1 for p in plans)
    assert all(int(np.prod(s)) < 1_000_000 for s in shapes)
    assert any(c.by_value for c in cases) and any(c.mask.max() > 1 and not c.by_value for c in cases)
    # the counts the table states without the reference are the reference's
    for c in cases:
        for conn in cc.CONNECTIVITIES:
            if c.expect is not None:
                assert ref.label(c.mask, conn, c.by_value)[1] == c.expect[conn], (c.name, conn)
    # the boundary pairs separate the three neighbourhoods
    kinds = {tuple(c.expect[k] for k in cc.CONNECTIVITIES) for c in cases if c.expect and c.mask.sum() == 2}
    assert kinds == {(1, 1, 1), (2, 1, 1), (2, 2, 1)}


def _by_size(labels, k):
    sizes = np.bincount(labels.ravel(), minlength=k + 1)[1:]
    table = np.zeros(k + 1, dtype=np.int32)
    table[1 + np.argsort(-sizes, kind="stable")] = np.arange(1, k + 1)
    return table[labels]


def test_the_comparison_sees_planted_mistakes():
    cases = {c.name: c for c in cc.build()}
    # 6 where 26 was asked
    m = cases["bernoulli_0.3_tiles"].mask
    want = ref.label(m, 26)
    with pytest.raises(AssertionError):
        ref.assert_same_labelling(*ref.label(m, 6), *want)
    with pytest.raises(AssertionError):
        ref.assert_same_labelling(*ref.label(m, 18), *want)
    # a dropped corner merge across one tile boundary: the two voxels stay two components
    c = cases["corner_01"]
    want = ref.label(c.mask, 26)
    assert want[1] == 1
    dropped = want[0].copy()
    dropped[tuple(np.argwhere(c.mask)[1])] = 2
    with pytest.raises(AssertionError):
        ref.assert_same_labelling(dropped, 2, *want)
    with pytest.raises(AssertionError):
        ref.assert_same_labelling(dropped, 1, *want)          # the right count over the wrong labels
    # numbering by size instead of by first voxel: the same partition, other ids
    want = ref.label(m, 26)
    resized = _by_size(*want)
    assert not np.array_equal(resized, want[0]) and np.array_equal(ref.renumber_by_first_voxel(resized)[0], want[0])
    with pytest.raises(AssertionError):
        ref.assert_same_labelling(resized, want[1], *want)
    # an off-by-one bounding box; overlap counted against the wrong mask
    other = cases["bernoulli_0.6_tiles"].mask
    table, peak = ref.stats(want[0], want[1], other, m.astype(np.float32))
    ref.assert_same_tables({"stats": table.copy(), "peak": peak.copy()}, {"stats": table, "peak": peak})
    box = table.copy()
    box[3, 7] += 1
    with pytest.raises(AssertionError):
        ref.assert_same_tables({"stats": box}, {"stats": table})
    wrong, _ = ref.stats(want[0], want[1], m)
    assert np.array_equal(wrong[:, 2:], table[:, 2:]) and np.array_equal(wrong[:, 0], table[:, 0])
    with pytest.raises(AssertionError):
        ref.assert_same_tables({"stats": wrong}, {"stats": table})
    # a lesion score off by one
    s = ref.lesion_scores(m, other, 26)
    ref.assert_same_scores(dict(s), s)
    with pytest.raises(AssertionError):
        ref.assert_same_scores(dict(s, lesions_detected=s["lesions_detected"] - 1), s)
