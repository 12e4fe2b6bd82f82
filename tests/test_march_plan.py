"""CPU suite: the launch plan of the marching 3x3x3 kernel (csrc/conv_march.hip) as mri3d_conv3d_march_plan_query answers it, held
to the rows of tests/march_cases.py.  Every row's declared plan numbers must be the query's (a change of seglen, nbuf or the
workgroup shape in conv_march_plan fails here by row id); the query must agree with mri3d_conv3d_march_supported,
mri3d_conv3d_march_stats_blocks and the workspace size; every refusal clause must answer MRI3D_ENOTSUP; and the table as a whole
must reach every corner of the kernel the parity suite exists for, computed from the queried plans (dropping a row fails the
closure test instead of thinning the coverage)."""
import ctypes

import pytest

import march_cases as mc
import march_run as run
from mri_epilepsy_diagnosis_amd import _lib, ops
from mri_epilepsy_diagnosis_amd._lib import BF16, F32, PASS_DGRAD, PASS_FWD, ConvGeom

EINVAL, ENOTSUP = -1, -2


@pytest.mark.parametrize("row,dtype", mc.PAIRS, ids=mc.IDS)
def test_declared_plan_numbers_are_the_querys(row, dtype):
    wrong = run.declared_mismatches(row, dtype, run.plans(row, dtype))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("row,dtype", mc.PAIRS, ids=mc.IDS)
def test_query_agrees_with_its_companions(row, dtype):
    L = _lib.lib()
    g = run.query_geom(row, dtype)
    for p, code in run.PASSES.items():
        info = _lib.MarchPlanInfo()
        rc = L.mri3d_conv3d_march_plan_query(ctypes.byref(g), code, 0, ctypes.byref(info))
        assert rc in (0, ENOTSUP), (row.id, dtype, p, rc)
        assert (rc == 0) == (L.mri3d_conv3d_march_supported(ctypes.byref(g), code) == 1), (row.id, dtype, p)
        if rc == 0:
            assert 0 < info.wp_bytes <= L.mri3d_conv3d_workspace_bytes(ctypes.byref(g), code), (row.id, dtype, p)
            assert 0 < info.smem_bytes <= 160 * 1024 and info.nbuf == (3 if info.chunks == 1 else 2)
            assert info.grid == info.blocks * info.gch * info.gcw * info.nseg * row.n
            assert info.wgh * info.wgw == 8 and (info.nseg - 1) * info.seglen < row.sp[0] <= info.nseg * info.seglen
    info = _lib.MarchPlanInfo()
    rc = L.mri3d_conv3d_march_plan_query(ctypes.byref(g), PASS_FWD, 1, ctypes.byref(info))
    blocks = L.mri3d_conv3d_march_stats_blocks(ctypes.byref(g))
    assert (rc == 0 and info.grid == blocks and blocks > 0) or (rc == ENOTSUP and blocks == 0), (row.id, dtype, rc, blocks)
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), PASS_DGRAD, 1, ctypes.byref(info)) == EINVAL      # no statistics there


def _geom(ci=16, co=16, sp=(4, 9, 17), k=3, s=1, p=1, d=1, x_ld=None, y_ld=None, dtype=F32):
    out = tuple((e + 2 * p - d * (k - 1) - 1) // s + 1 for e in sp)
    return ConvGeom(1, *sp, ci, *out, co, k, k, k, s, s, s, p, p, p, d, d, d, x_ld or ci, y_ld or co, dtype)


REFUSALS = {
    # clause: (geometry, pass, stats, what mri3d_conv3d_march_supported says)
    "stride 2": (_geom(s=2), PASS_FWD, 0, 0),
    "dilation 2": (_geom(d=2, p=2), PASS_FWD, 0, 0),
    "kernel size 1": (_geom(k=1, p=0), PASS_FWD, 0, 0),
    "kernel size 5": (_geom(k=5, p=2), PASS_DGRAD, 0, 0),
    "Kc % 8 (forward ci = 12)": (_geom(ci=12), PASS_FWD, 0, 0),
    "Kc % 8 (data gradient co = 12)": (_geom(co=12), PASS_DGRAD, 0, 0),
    "input pitch % 4 (fp32)": (_geom(x_ld=18), PASS_FWD, 0, 0),
    "input pitch % 8 (bf16)": (_geom(x_ld=20, dtype=BF16), PASS_FWD, 0, 0),
    "output pitch % 4 (fp32)": (_geom(y_ld=18), PASS_FWD, 0, 0),
    "output pitch % 8 (bf16)": (_geom(y_ld=20, dtype=BF16), PASS_FWD, 0, 0),
    "output pitch of the data gradient % 8 (bf16)": (_geom(x_ld=20, dtype=BF16), PASS_DGRAD, 0, 0),
    "Nc < 8": (_geom(co=4), PASS_FWD, 0, 0),
    "Nc % 8 (bf16)": (_geom(co=12, dtype=BF16), PASS_FWD, 0, 0),
    "five chunks (fp32 Kc = 40)": (_geom(ci=40), PASS_FWD, 0, 0),
    "five chunks (bf16 Kc = 72)": (_geom(ci=72, dtype=BF16), PASS_FWD, 0, 0),
    "five chunks (data gradient, fp32 co = 40)": (_geom(co=40), PASS_DGRAD, 0, 0),
    "nine statistics blocks": (_geom(ci=8, co=136), PASS_FWD, 1, 1),
}


@pytest.mark.parametrize("clause", sorted(REFUSALS))
def test_refusal_clauses_answer_enotsup(clause):
    L = _lib.lib()
    g, code, stats, supported = REFUSALS[clause]
    info = _lib.MarchPlanInfo()
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), code, stats, ctypes.byref(info)) == ENOTSUP, clause
    assert L.mri3d_conv3d_march_supported(ctypes.byref(g), code) == supported, clause
    if stats:
        assert L.mri3d_conv3d_march_stats_blocks(ctypes.byref(g)) == 0, clause
        assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), code, 0, ctypes.byref(info)) == 0 and info.blocks == 9
    with pytest.raises(_lib.Mri3dError):
        ops.conv_march_plan(g, code, bool(stats))


def test_the_clauses_refuse_one_step_from_a_served_geometry():
    """each clause above differs from this geometry in the one thing it names"""
    for dtype in (F32, BF16):
        for code in (PASS_FWD, PASS_DGRAD):
            assert ops.conv_march_plan(_geom(dtype=dtype), code)["grid"] == 1
    assert ops.conv_march_plan(_geom(ci=8, co=128), PASS_FWD, True)["blocks"] == 8
    assert ops.conv_march_plan(_geom(ci=32), PASS_FWD)["chunks"] == 4 and ops.conv_march_plan(_geom(ci=64, dtype=BF16), PASS_FWD)["chunks"] == 4
    assert ops.conv_march_plan(_geom(x_ld=20, y_ld=20), PASS_FWD)["grid"] == 1 and ops.conv_march_plan(_geom(x_ld=24, y_ld=24, dtype=BF16), PASS_DGRAD)["grid"] == 1


def test_query_validates_its_arguments():
    L = _lib.lib()
    g, info = _geom(), _lib.MarchPlanInfo()
    assert L.mri3d_conv3d_march_plan_query(None, PASS_FWD, 0, ctypes.byref(info)) == EINVAL
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), PASS_FWD, 0, None) == EINVAL
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), 2, 0, ctypes.byref(info)) == EINVAL            # no weight gradient here
    bad = _geom()
    bad.dout += 1
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(bad), PASS_FWD, 0, ctypes.byref(info)) == EINVAL


# ---------------------------------------------------------------------------------------------- what the table reaches
def wait_counts(pl, row, dtype):
    """the values of `younger` (the N of s_waitcnt vmcnt(N)) the items of every active wave of the launch take, restated from the
    item loop of conv_march_body: 6 pieces of the next item where the DMA leads by two, the stores of the plane just completed"""
    D, H, _ = row.sp
    per_plane = 4 if dtype == "bf16" else 8
    seen = set()
    for seg in range(pl["nseg"]):
        dlo = seg * pl["seglen"]
        dhi = min(dlo + pl["seglen"], D)
        plo, phi = max(dlo - 1, 0), min(dhi, D - 1)
        nitems = (phi - plo + 1) * pl["chunks"]
        for h0 in range(0, H, 8):
            nstores = per_plane if h0 + 8 <= H else 0
            for it in range(nitems):
                p, c = plo + it // pl["chunks"], it % pl["chunks"]
                stored = c == 0 and p - 2 >= dlo
                seen.add((6 if pl["nbuf"] == 3 and it + 1 < nitems else 0) + (nstores if stored else 0))
    return seen


def test_the_table_reaches_every_corner():
    reached = {d: {"shapes": set(), "nbuf": set(), "chunks": set(), "waits": set(), "residues": set(), "dma": set(), "segments": set(),
                   "wait cells": set()} for d in mc.DTYPES}
    flags = {d: set() for d in mc.DTYPES}
    for row, dtype in mc.PAIRS:
        pls = run.plans(row, dtype)
        for p, pl in pls.items():
            if pl is None:
                continue
            r = reached[dtype]
            D, H, W = row.sp
            r["shapes"].add((pl["wgh"], pl["wgw"]))
            r["nbuf"].add(pl["nbuf"])
            r["chunks"].add(pl["chunks"])
            r["waits"] |= wait_counts(pl, row, dtype)
            if D >= 4:
                r["wait cells"].add((pl["nbuf"], H % 8 == 0))
            r["residues"] |= {(s * pl["seglen"] - 1) % 3 for s in range(1, pl["nseg"])}
            r["dma"].add("constant offsets" if pl["whole_chunks"] and not (row.split and p == "fwd") else "offsets per piece")
            r["segments"] |= {"only"} if pl["nseg"] == 1 else {"first", "last"} | ({"interior"} if pl["nseg"] > 2 else set())
            nc = row.co if p == "fwd" else row.ci
            f = flags[dtype]
            if pl["wgh"] * pl["gch"] * 8 >= H + 8 or pl["wgw"] * pl["gcw"] * 16 >= W + 16:
                f.add("an inactive wave")
            if nc % 16:
                f.add("a half-filled last output block")
            if D % pl["seglen"]:
                f.add("a shorter last segment")
            if row.n > 1 and pl["nseg"] > 1 and pl["blocks"] > 1:
                f.add("the whole decode: samples, segments and output blocks")
            if pl["grid"] % 8:
                f.add("a grid that is no multiple of 8" if pl["grid"] < 8 else "a grid above 8 that is no multiple of 8")
            if row.stats and p == "fwd":
                f.add("statistics")
                if pl["blocks"] == 8:
                    f.add("statistics of eight output blocks")
                if row.split:
                    f.add("statistics of a split forward")
            if row.split:
                f.add("a split " + p)
                if p == "fwd" and not pl["whole_chunks"]:
                    f.add("a second tensor that ends in half a chunk")
            if p == "fwd":
                f.add("bias" if row.bias else "no bias")
                f.add(("statistics" if row.stats else "plain") + (" with bias" if row.bias else " without bias"))
            if row.layout:
                f |= {"pitched " + k for k in row.layout}
    want_waits = {"f32": {0, 6, 8, 14}, "bf16": {0, 4, 6, 10}}
    for d in mc.DTYPES:
        r = reached[d]
        print(d, {k: sorted(v) for k, v in r.items()}, sorted(flags[d]))
        assert r["shapes"] == {(4, 2), (2, 4), (8, 1), (1, 8)}, (d, r["shapes"])
        assert r["nbuf"] == {2, 3} and r["chunks"] == {1, 2, 3, 4}, (d, r["nbuf"], r["chunks"])
        assert r["waits"] == want_waits[d], (d, r["waits"])                      # every count the type can take
        assert r["wait cells"] == {(2, True), (2, False), (3, True), (3, False)}, (d, r["wait cells"])
        assert r["residues"] == {0, 1, 2}, (d, r["residues"])
        assert r["dma"] == {"constant offsets", "offsets per piece"}, (d, r["dma"])
        assert r["segments"] == {"only", "first", "interior", "last"}, (d, r["segments"])
        missing = {"an inactive wave", "a half-filled last output block", "a shorter last segment", "a grid that is no multiple of 8",
                   "a grid above 8 that is no multiple of 8", "the whole decode: samples, segments and output blocks", "statistics of eight output blocks",
                   "statistics of a split forward", "a split fwd", "a split dgrad", "plain with bias", "plain without bias",
                   "statistics with bias", "statistics without bias", "pitched x", "pitched y", "pitched x2"} - flags[d]
        assert not missing, (d, missing)
    assert "a second tensor that ends in half a chunk" in flags["bf16"]            # (fp32 chunks are 8 channels: Kc % 8 == 0 fills them)
    assert want_waits["f32"] | want_waits["bf16"] == {0, 4, 6, 8, 10, 14}          # the six cases of the kernel's wait
    # the depths the kernel's plane bookkeeping distinguishes
    assert {1, 2, 3} <= {r.sp[0] for r in mc.ROWS}
    # fp32 output blocks that end on a quad inside a block
    assert {12, 20} <= {r.co for r in mc.ROWS if mc.runs(r, "f32", "fwd")}


def test_dispatcher_flag():
    """1 for the full-resolution layers tests/conv_cases.py pins to "march", 0 for a small volume the explicit entry points take"""
    full = (160, 192, 160)
    for dtype in (F32, BF16):
        for code in (PASS_FWD, PASS_DGRAD):
            pl = ops.conv_march_plan(_geom(sp=full, dtype=dtype), code)
            assert pl["dispatcher"] == 1 and pl["blocks"] == 1 and pl["grid"] >= 192, (dtype, code, pl)
        assert ops.conv_march_plan(_geom(sp=full, dtype=dtype), PASS_FWD, True)["dispatcher"] == 1
    # three output blocks: only as the data gradient (of the decoder's 48 -> 16 layer), never as a forward
    assert ops.conv_march_plan(_geom(ci=16, co=48, sp=full, dtype=BF16), PASS_FWD)["dispatcher"] == 0
    assert ops.conv_march_plan(_geom(ci=48, co=16, sp=full, dtype=BF16), PASS_DGRAD)["dispatcher"] == 1
    small = ops.conv_march_plan(_geom(dtype=BF16), PASS_FWD)
    assert small["dispatcher"] == 0 and small["grid"] == 1
    assert ops.conv_march_plan(_geom(sp=(40, 48, 40)), PASS_FWD)["dispatcher"] == 0            # fp32 below 4 Mi voxels
