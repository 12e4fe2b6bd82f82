"""CPU suite: the launch plans of the 3x3x3 MFMA convolution family (csrc/conv_mfma.hip, csrc/conv_mfma_wgrad.hip) as
mri3d_conv3d_mfma_plan_query answers them, held to the rows of tests/mfma_cases.py.  Every row's declared plan numbers and route
names must be the library's (a threshold that moves in fwd_route, direct_plan or mfma_wgrad_plan fails here by row id); the query
must answer exactly where mri3d_conv3d_route names a kernel of the two files, agree with the workspace and statistics queries and
with itself; and the table as a whole must serve every route name of the two files and reach the corners the parity suite exists
for, computed from the queried plans (dropping a row fails the coverage tests instead of thinning the coverage)."""
import ctypes

import pytest

import mfma_cases as mc
import mfma_run as run
from mri_epilepsy_diagnosis_amd import _lib, ops
from mri_epilepsy_diagnosis_amd._lib import PASS_DGRAD, PASS_FWD, PASS_WGRAD

EINVAL, ENOTSUP = -1, -2
OWN_WORDS = ("tiled", "tiled_n8", "direct", "cin1", "wgrad3", "wgrad4", "bf16", "bf16t", "wgrad6")


@pytest.mark.parametrize("row,dtype", mc.PAIRS, ids=mc.IDS)
def test_declared_plan_numbers_are_the_querys(row, dtype):
    wrong = run.declared_mismatches(row, dtype, run.plans(row, dtype))
    assert not wrong, "\n".join(wrong)


def _cdiv(a, b):
    return -(-a // b)


@pytest.mark.parametrize("row,dtype", mc.PAIRS, ids=mc.IDS)
def test_query_answers_where_the_route_names_the_family_and_agrees_with_its_companions(row, dtype):
    L = _lib.lib()
    g = run.geom(row, dtype)
    for p in ("fwd", "dgrad", "wgrad"):
        for stats in ((False, True) if p == "fwd" else (False,)):
            for al in (16, 8):
                kw = dict(stats=stats, bias=False, split=row.split, second_ld=run.width(row, "x2") if row.split else 0, align=al)
                name = ops.conv_route(g, run.PASSES[p], **kw)
                info = _lib.ConvMfmaPlanInfo()
                ctypes.memset(ctypes.byref(info), 0x5A, ctypes.sizeof(info))
                rc = L.mri3d_conv3d_mfma_plan_query(ctypes.byref(g), run.PASSES[p], int(stats), 0, row.split, kw["second_ld"], al, al, ctypes.byref(info))
                own = name.split()[0] in OWN_WORDS
                assert rc == (0 if own else ENOTSUP), (row.id, dtype, p, stats, al, name, rc)
                if not own:
                    assert bytes(info) == b"\x5a" * ctypes.sizeof(info), "a refusing query wrote to its result"
                    assert al == 16 or name.split()[0] in ("generic", "pointwise", "none")
                    continue
                q = ops.conv_mfma_plan(g, run.PASSES[p], **kw)
                what = (row.id, dtype, p, stats, name, q)
                assert name.split()[0] == q["kernel"], what
                assert 0 < q["workspace_bytes"] <= L.mri3d_conv3d_workspace_bytes(ctypes.byref(g), run.PASSES[p]), what
                assert q["min_tasks"] <= q["max_tasks"] and q["min_tasks"] * q["grid"] <= q["units"] * max(q["cit"] * q["cob"], 1), what
                if p == "fwd":
                    blocks = L.mri3d_conv3d_fwd_cat_stats_blocks(ctypes.byref(g), row.split, kw["second_ld"]) if row.split else \
                        L.mri3d_conv3d_fwd_stats_blocks(ctypes.byref(g))
                    assert q["stats_blocks"] == (q["grid"] if stats else 0) and (not stats or blocks == q["grid"]), what
                if q["kernel"] in ("tiled", "tiled_n8"):
                    assert name == ("tiled_n8" if q["kernel"] == "tiled_n8" else "tiled nt%d%s" % (q["nt"], " stats" if stats else "")), what
                    assert q["ntiles"] == row.n * q["tiles_d"] * q["tiles_h"] * q["tiles_w"] and q["units"] == q["ntiles"] * q["gy"], what
                    assert q["grid"] == min(q["units"], 512) and q["ntt"] == q["nt"] * q["gy"], what
                    assert q["max_tasks"] >= _cdiv(q["units"], q["grid"]) and q["max_tasks"] * q["grid"] >= q["units"], what
                    assert (q["tile_d"], q["tile_h"], q["tile_w"]) == (4, 8, 16) and q["ck"] == (16 if dtype == "bf16" else 8), what
                elif q["kernel"] == "direct":
                    assert name == "direct nt%d mode%d split%d" % (q["nt"], q["mode"], q["split"]), what
                    assert q["units"] == q["ntiles"] * q["gy"] and q["split"] == (1 if q["units"] < 1024 else 0), what
                    assert q["grid"] == (q["units"] if q["split"] else _cdiv(q["units"], 4)) and q["ntt"] == q["nt"] * q["gy"], what
                    assert q["mode"] == (1 if p == "dgrad" and row.stride > 1 else 0), what
                else:
                    assert name == q["kernel"] + (" ci8" if q["ci8"] else "") + (" co8" if q["co8"] else ""), what
                    assert q["grid"] == q["p"] * q["cit"] * q["cob"] and q["p"] == min(max(512 // (q["cit"] * q["cob"]), 1), q["ntiles"]), what
                    assert q["ntiles"] == row.n * q["tiles_d"] * q["tiles_h"] * q["tiles_w"] == q["units"], what
                    assert q["chain"] == q["max_tasks"] * q["tile_d"] * q["tile_h"] * q["tile_w"] // 4, what
                    assert q["max_tasks"] * q["p"] >= q["ntiles"] >= q["min_tasks"] * q["p"] and q["max_tasks"] >= _cdiv(q["ntiles"], q["p"]), what
                    assert q["workspace_bytes"] == q["p"] * q["cit"] * q["cob"] * (q["tg"] + 1) * 1024, what
                    assert (q["segl"] > 0) == (q["kernel"] == "bf16t") and (q["kernel"] != "bf16t" or q["tile_d"] == q["segl"]), what


def test_query_validates_its_arguments():
    L = _lib.lib()
    row = mc.row("args", 16, 16, (5, 9, 17))
    g, info = run.geom(row, "bf16"), _lib.ConvMfmaPlanInfo()
    q = lambda *a: L.mri3d_conv3d_mfma_plan_query(*a)      # noqa: E731
    assert q(ctypes.byref(g), PASS_FWD, 0, 0, 0, 0, 16, 16, ctypes.byref(info)) == 0 and info.kernel == 1
    assert q(None, PASS_FWD, 0, 0, 0, 0, 16, 16, ctypes.byref(info)) == EINVAL
    assert q(ctypes.byref(g), PASS_FWD, 0, 0, 0, 0, 16, 16, None) == EINVAL
    assert q(ctypes.byref(g), 3, 0, 0, 0, 0, 16, 16, ctypes.byref(info)) == EINVAL
    assert q(ctypes.byref(g), PASS_DGRAD, 1, 0, 0, 0, 16, 16, ctypes.byref(info)) == EINVAL          # no statistics there
    assert q(ctypes.byref(g), PASS_WGRAD, 1, 0, 0, 0, 16, 16, ctypes.byref(info)) == EINVAL
    assert q(ctypes.byref(g), PASS_FWD, 0, 0, -16, 0, 16, 16, ctypes.byref(info)) == EINVAL
    bad = run.geom(row, "bf16")
    bad.dout += 1
    assert q(ctypes.byref(bad), PASS_FWD, 0, 0, 0, 0, 16, 16, ctypes.byref(info)) == EINVAL
    with pytest.raises(_lib.Mri3dError):
        ops.conv_mfma_plan(g, PASS_FWD, align=8)
    assert ops.conv_mfma_plan(g, PASS_FWD)["kernel"] == "tiled" and set(ops.MFMA_KERNELS.values()) == set(OWN_WORDS)


def test_the_marching_kernels_layers_are_not_this_querys():
    """a full-resolution bf16 layer is the marching kernel's by the dispatcher's choice: another file, its own query"""
    row = mc.row("full", 16, 16, (160, 192, 160))
    assert run.route(row, "bf16", "fwd").split()[0] == "march" and run.plan(row, "bf16", "fwd") is None
    assert run.plan(row, "bf16", "wgrad")["kernel"] == "bf16"          # (the weight gradient of the same layer is this family's)


# ---------------------------------------------------------------------------------------------- what the table reaches
def _served():
    """{storage type: {route name: [row ids]}} over the passes the rows run"""
    out = {d: {} for d in mc.DTYPES}
    for row, dtype in mc.PAIRS:
        for p, pl in run.plans(row, dtype).items():
            if pl is not None and mc.runs(row, dtype, p):
                out[dtype].setdefault(pl["route"], []).append(row.id)
    return out


def test_every_route_name_of_the_two_files_is_served_in_every_storage_type_that_has_it():
    """The names of include/mri3d.h's grammar: tiled nt{1,2}[ stats], tiled_n8, direct nt{1,2,4} mode{0,1} split{0,1}, cin1, wgrad3,
    wgrad4, bf16, bf16t, wgrad6[ ci8][ co8].  Of these mri3d_conv3d_route cannot produce: direct nt{2,4} split1 (direct_plan keeps
    nt > 1 only from 4096 units, and splits a unit's taps over the waves only below 1024); wgrad6 ci8 without co8 (mfma_wgrad_plan sets
    ci8 only inside the co == 8 clause); and per storage type: wgrad6 is an fp32 kernel, wgrad4, bf16 and bf16t are bf16 kernels."""
    direct = {"direct nt%d mode%d split%d" % (nt, m, s) for nt in (1, 2, 4) for m in (0, 1) for s in (0, 1)} - \
        {"direct nt%d mode%d split1" % (nt, m) for nt in (2, 4) for m in (0, 1)}
    common = {"tiled nt1", "tiled nt2", "tiled nt1 stats", "tiled nt2 stats", "tiled_n8", "cin1", "wgrad3"} | direct
    want = {"f32": common | {"wgrad6", "wgrad6 co8", "wgrad6 ci8 co8"}, "bf16": common | {"wgrad4", "bf16", "bf16t"}}
    got = _served()
    for d in mc.DTYPES:
        print(d, {k: len(v) for k, v in sorted(got[d].items())})
        assert not want[d] - set(got[d]), (d, "no row serves", sorted(want[d] - set(got[d])))
        assert not set(got[d]) - want[d], (d, "names outside the grammar", sorted(set(got[d]) - want[d]))


def test_the_table_reaches_every_corner():
    flags = {d: set() for d in mc.DTYPES}
    for row, dtype in mc.PAIRS:
        f = flags[dtype]
        for p, q in run.plans(row, dtype).items():
            if q is None:
                f.add("refused " + p if p in row.refused.get(dtype, ()) else "leaves the family: " + p)
                continue
            k = q["kernel"]
            pitched = sorted(n for n in row.layout)
            f |= {"%s pitched %s" % (k, n) for n in pitched}
            if k in ("tiled", "tiled_n8"):
                D, H, W = row.sp
                f.add("%s %s" % (k, p))
                f.add("tiled chunks %d" % q["chunks"])
                if q["partial_chunk"]:
                    f.add("tiled half-filled last chunk" + (" from a pitched buffer" if (p == "fwd" and "x" in row.layout) else ""))
                f.add("tiled nt%d gy%d" % (q["nt"], q["gy"]))
                if (row.co if p == "fwd" else row.ci) % 16 and k == "tiled":
                    f.add("tiled half-empty n-tile")
                if (D, H, W) == (4, 8, 16):
                    f.add("tiled exact tile")
                if D % 4 and H % 8 and W % 16 and q["ntiles"] > 1:
                    f.add("tiled ragged in d, h and w")
                if W % 16 == 1 and q["tiles_w"] == 2:
                    f.add("tiled one voxel in the second w tile")
                if D < 4 and H < 8 and W < 16:
                    f.add("tiled below one tile")
                if q["grid"] == q["units"] < 512:
                    f.add("tiled grid == units")
                if q["grid"] == 512 and q["max_tasks"] == 2 and q["min_tasks"] == 1:
                    f.add("tiled second tile for some workgroups")
                if q["grid"] % 8:
                    f.add("tiled grid no multiple of 8")
                if q["min_tasks"] == 0:
                    f.add("tiled workgroups without a tile" + (" with statistics" if row.stats and p == "fwd" else ""))
                if row.stats and p == "fwd":
                    f.add("stats " + ("with bias" if row.bias else "without bias"))
                    if q["ntt"] == 8:
                        f.add("stats of 128 channels")
                    if row.n > 1:
                        f.add("stats n > 1")
                    if row.split:
                        f.add("stats with a split")
                if row.split:
                    f.add("tiled split %s %d+%d" % (p, row.split, row.ci - row.split))
            elif k == "direct":
                f.add("direct nt%d%s" % (q["nt"], " narrowed" if q["ntt"] % 4 == 0 and q["nt"] < 4 else ""))
                f.add("direct split%d %s" % (q["split"], "1023 units" if q["units"] == 1023 else "1024 units" if q["units"] == 1024 else ""))
                f.add("direct mode%d stride %d" % (q["mode"], row.stride))
                if row.sp[2] <= 8 and row.stride == 1:
                    f.add("direct narrow")
                if (row.n * row.sp[0] * row.sp[1] * row.sp[2]) % 16 and row.n > 1 and row.stride == 1:
                    f.add("direct M-tile over two samples")
                if q["partial_chunk"]:
                    f.add("direct Kc %d" % (row.ci if p == "fwd" else row.co))
                if (row.co if p == "fwd" else row.ci) == 8:
                    f.add("direct Nc 8")
                if row.stride > 1:
                    f.add("direct strided %s extents" % ("odd" if any(e % 2 for e in row.sp) else "even"))
                if q["wbn"] > 1:
                    f.add("direct wbn > 1")
            else:
                f.add("wgrad " + q["route"])
                f.add("%s %s dbias" % (k, "with" if row.dbias else "without"))
                if row.split:
                    f.add("%s split" % k)
                if q["cit"] > 1:
                    f.add("%s cit > 1" % k)
                if q["cob"] > 1 and row.co % 16:
                    f.add("%s half-empty output block" % k)
                if q["partial_chunk"]:
                    f.add("%s partial ci-tile" % k)
                if q["p"] == q["ntiles"]:
                    f.add("walk p == ntiles")
                if q["p"] < q["ntiles"] and q["max_tasks"] > q["min_tasks"] > 0:
                    f.add("walk uneven")
                if q["max_tasks"] > 2:
                    f.add("walk more than two tiles")
                if q["min_tasks"] == 0:
                    f.add("walk empty workgroups")
                if q["p"] % 8:
                    f.add("walk p no multiple of 8")
                if k == "bf16t":
                    f.add("bf16t segl %d" % q["segl"])
                    if row.sp[0] % q["segl"] and row.sp[0] > q["segl"]:
                        f.add("bf16t shorter last segment")
                    if row.sp[0] == 8:
                        f.add("bf16t d == 8")
    common = {"tiled fwd", "tiled dgrad", "tiled_n8 fwd", "tiled_n8 dgrad", "tiled chunks 1", "tiled chunks 2", "tiled exact tile",
              "tiled ragged in d, h and w", "tiled one voxel in the second w tile", "tiled nt1 gy1", "tiled nt1 gy3", "tiled nt2 gy1",
              "tiled nt2 gy2", "tiled half-empty n-tile", "tiled grid == units", "tiled second tile for some workgroups", "tiled grid no multiple of 8",
              "tiled workgroups without a tile with statistics", "stats with bias", "stats without bias", "stats of 128 channels", "stats n > 1",
              "stats with a split", "tiled split fwd 16+8", "tiled split fwd 16+16", "tiled split dgrad 16+16", "tiled split dgrad 16+8",
              "tiled pitched x", "tiled pitched y", "tiled pitched x2", "refused fwd", "refused dgrad", "refused wgrad",
              "direct mode0 stride 2", "direct mode1 stride 2", "direct mode0 stride 3", "direct mode1 stride 3", "direct strided odd extents",
              "direct strided even extents", "direct wbn > 1", "direct Kc 12", "direct Kc 20", "direct Nc 8", "direct nt1", "direct nt2", "direct nt4",
              "direct pitched x", "direct pitched y", "wgrad cin1", "wgrad wgrad3", "wgrad3 cit > 1", "wgrad3 with dbias", "wgrad3 without dbias",
              "walk p == ntiles", "walk uneven", "walk empty workgroups", "walk p no multiple of 8",
              "leaves the family: fwd", "leaves the family: dgrad", "leaves the family: wgrad"}
    want = {
        "f32": common | {"tiled chunks 6", "direct narrow", "direct M-tile over two samples", "direct nt1 narrowed", "direct nt2 narrowed",
                         "direct split1 1023 units", "direct split0 1024 units", "direct mode0 stride 1", "wgrad wgrad6", "wgrad wgrad6 co8",
                         "wgrad wgrad6 ci8 co8", "wgrad6 cit > 1", "wgrad6 half-empty output block", "wgrad6 split", "wgrad6 with dbias",
                         "wgrad6 without dbias", "wgrad6 pitched x", "wgrad6 pitched y", "wgrad6 pitched x2", "walk more than two tiles"},
        "bf16": common | {"tiled half-filled last chunk", "tiled half-filled last chunk from a pitched buffer", "tiled below one tile",
                          "tiled workgroups without a tile", "wgrad wgrad4", "wgrad bf16", "wgrad bf16t", "bf16 partial ci-tile", "bf16 cit > 1",
                          "bf16 half-empty output block", "bf16 split", "bf16 with dbias", "bf16 without dbias", "bf16t split", "bf16t with dbias",
                          "bf16t without dbias", "bf16t segl 20", "bf16t segl 40", "bf16t shorter last segment", "bf16t d == 8", "bf16 pitched x",
                          "bf16 pitched y", "bf16 pitched x2", "wgrad4 pitched y"},
    }
    for d in mc.DTYPES:
        print(d, sorted(flags[d]))
        assert not want[d] - flags[d], (d, sorted(want[d] - flags[d]))
