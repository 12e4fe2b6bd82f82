"""CPU suite: which kernel every pool and upsample parity case runs on, and which kernels have no case.

mri3d_maxpool3d_route / mri3d_upsample3d_route answer, without a device, from the launch plan the entry points launch by (one plan
function per pass in csrc/resample.hip).  So the coverage of the GPU parity cases of tests/resample_cases.py is checked here:

  a. every row reaches the kernel it declares, queried with the alignments its tensors have on the device;
  b. every instantiation name (VOCABULARY, hand-written) is reached by a row: UNREACHED, exactly the rest, is empty;
  c. a sweep over dtypes, channels, extents, pitches, alignments and modes finds no name outside VOCABULARY, no 16-byte bf16 kernel
     on a tensor that is not 16-byte aligned and pitched in octets, and no vector kernel on channels that are not whole quads;
  d. the geometries at which the x2 forward halves its segment length keep their kernel (the length itself is a run-time argument,
     not part of a name);
  e. every parity row (PARITY_POOL, PARITY_UP) reaches the names AND the plan numbers it declares (ops.pool_plan / ops.upsample_plan),
     and is there for what its section says: more items than workgroups, slabs that are parts of a plane, its segment length;
  f. a sweep of both plan queries finds no plan corner — kernel x vec x segment-length class x (items > grid) x chunked — that no
     parity row reaches;
  g. geometries past the 32-bit limits of the x2 kernels and of the line-contiguous pool decline to the kernels without them
     (host only: nothing is allocated)."""
import itertools

import pytest

import resample_cases as rc
import resample_run as run
from mri_epilepsy_diagnosis_amd import ops
from mri_epilepsy_diagnosis_amd._lib import BF16, F32, PASS_DGRAD, PASS_FWD, UP_NEAREST, UP_TRILINEAR, PoolGeom, UpGeom

TYPES = {"f32": F32, "bf16": BF16}
_VECS = {"f32": (1, 4), "bf16": (1, 4, 8)}       # channels per lane item: 16-byte items of 8 exist for bf16 only

# ---- b. every instantiation csrc/resample.hip launches, by pass (include/mri3d.h documents the names)
VOCABULARY = {
    ("pool", PASS_FWD): ["maxpool2_fwd<%s,%d>" % (t, v) for t in TYPES for v in _VECS[t] if v >= 4] +
                        ["maxpool_fwd<%s,%d>" % (t, v) for t in TYPES for v in _VECS[t]],
    ("pool", PASS_DGRAD): ["maxpool_bwd<%s,%d>%s" % (t, v, add) for t in TYPES for v in _VECS[t] for add in ("", "+add")],
    ("up", PASS_FWD): ["upsample2x_fwd_march<%s,%d,%d>" % (t, v, n) for t in TYPES for v in _VECS[t] if v >= 4 for n in (1, 2, 4, 8)] +
                      ["upsample_fwd<%s,%d>" % (t, v) for t in TYPES for v in (1, 4)],
    ("up", PASS_DGRAD): ["upsample2x_bwd_march<%s>" % t for t in TYPES] + ["upsample2x_bwd<%s>" % t for t in TYPES] +
                        ["upsample_nearest_int_bwd<%s,%d>" % (t, s) for t in TYPES for s in (2, 4)] +
                        ["tables+upsample_bwd<%s,%d>" % (t, v) for t in TYPES for v in (1, 4)],
}
# what no row of tests/resample_cases.py reaches: nothing (PARITY_POOL_UNREACHED / PARITY_UP_UNREACHED took the last eleven)
UNREACHED = ()


def pool_geom(dtype, c, sp, k, s, x_ld=None, y_ld=None, n=rc.N):
    out = [(i - k) // s + 1 for i in sp]
    return PoolGeom(n, *sp, *out, c, k, k, k, s, s, s, 0, 0, 0, x_ld or c, y_ld or c, TYPES[dtype])


def up_geom(dtype, c, sp, mode, size=None, scale=None, ac=None, x_ld=None, y_ld=None, n=rc.N):
    """The UpGeom `ops.upsample3d` builds (the ratios are torch's: the given scale, in / out for a size, corners for align_corners)."""
    out = tuple(size) if size is not None else tuple(int(i * scale) for i in sp)
    ratios = [((i - 1) / (o - 1) if o > 1 else 0.0) if mode == "trilinear" and ac else (1.0 / scale if scale is not None else i / o)
              for i, o in zip(sp, out)]
    return UpGeom(n, *sp, *out, c, x_ld or c, y_ld or c, UP_NEAREST if mode == "nearest" else UP_TRILINEAR, 1 if ac else 0, *ratios,
                  TYPES[dtype])


def _slice_align(pad, esz):
    """ptr_align of the last channels of a freshly allocated buffer `pad` channels wider"""
    off = pad * esz
    return min(16, off & -off) if off else 16


def row_routes():
    """(row id, family, pass, declared name, answered name) of every row, as the GPU tests run it"""
    for r in rc.POOL_ROWS:
        g = pool_geom(r.dtype, r.c, r.sp, r.k, r.s)
        yield "pool/" + r.id, "pool", PASS_FWD, r.fwd, ops.pool_route(g, PASS_FWD)
        yield "pool/" + r.id, "pool", PASS_DGRAD, r.bwd, ops.pool_route(g, PASS_DGRAD)
    for r, dtype in itertools.product(rc.POOL_SKIP, TYPES):
        g, rid = pool_geom(dtype, r.c, r.sp, 2, 2), "skip/%s/%s" % (r.id, dtype)
        yield rid, "pool", PASS_FWD, r.fwd[dtype], ops.pool_route(g, PASS_FWD)
        # dskip is the pitched slice, or (one output used) dense zeros; dy, dx and the index bytes are fresh allocations
        yield rid, "pool", PASS_DGRAD, r.bwd[dtype], ops.pool_route(g, PASS_DGRAD, addend_ld=r.c + r.pad,
                                                                     align=_slice_align(r.pad, 2 if dtype == "bf16" else 4))
        yield rid, "pool", PASS_DGRAD, r.bwd[dtype], ops.pool_route(g, PASS_DGRAD, addend_ld=r.c)
    for r in rc.UP_ROWS:
        g = up_geom(r.dtype, r.c, r.sp, r.mode, r.size, r.scale, r.ac)
        yield "up/" + r.id, "up", PASS_FWD, r.fwd, ops.upsample_route(g, PASS_FWD)
        yield "up/" + r.id, "up", PASS_DGRAD, r.bwd, ops.upsample_route(g, PASS_DGRAD)
    for r, dtype in rc.PARITY_PAIRS:
        got, family = run.plans(r, dtype), "pool" if run.is_pool(r) else "up"
        yield "parity/%s/%s" % (r.id, dtype), family, PASS_FWD, r.fwd[dtype], got["fwd"][0]
        yield "parity/%s/%s" % (r.id, dtype), family, PASS_DGRAD, r.bwd[dtype], got["bwd"][0]


# ---- a.
def test_every_row_reaches_the_route_it_declares():
    wrong = ["%s: declares %s, runs %s" % (rid, want, got) for rid, _, _, want, got in row_routes() if want != got]
    assert not wrong, "%d row(s) left their kernel:\n  %s" % (len(wrong), "\n  ".join(wrong))


# ---- b.
def test_every_instantiation_has_a_row_or_is_listed_as_unreached():
    names = [n for v in VOCABULARY.values() for n in v]
    assert len(names) == len(set(names)) == 46
    reached = {got for _, _, _, _, got in row_routes()}
    assert reached <= set(names)
    assert sorted(set(names) - reached) == sorted(UNREACHED)
    assert UNREACHED == ()


# ---- c.
def _vec(name):
    """channels per lane item of the kernel `name`"""
    args = name[name.index("<") + 1:name.index(">")].split(",")
    if name.startswith(("upsample2x_bwd", "upsample_nearest_int_bwd")):
        return 4
    return int(args[1])


CHANNELS = (1, 3, 4, 8, 12, 16, 20, 24, 36, 40, 64)
ALIGNS = (4, 8, 16)


def _check(name, family, pass_, dtype, c, pitches, align, idx_align=16):
    assert name in VOCABULARY[(family, pass_)], name
    assert ("<%s" % dtype) in name
    if _vec(name) == 8:
        assert dtype == "bf16" and align == 16 and idx_align >= 8 and all(ld % 8 == 0 for ld in pitches) and c % 8 == 0, (name, c, pitches, align)
    if c % 4 != 0:
        assert _vec(name) == 1, (name, c)
    if _vec(name) == 4:
        assert all(ld % 4 == 0 for ld in pitches) and align >= (8 if dtype == "bf16" else 16), (name, c, pitches, align)


@pytest.mark.parametrize("dtype", list(TYPES))
def test_pool_sweep_stays_in_the_vocabulary(dtype):
    seen = set()
    for c, sp, (k, s), pad, align, idx_align in itertools.product(CHANNELS, ((5, 7, 9), (4, 6, 8), (8, 8, 4)), ((2, 2), (4, 2)), (0, 4), ALIGNS, ALIGNS):
        g = pool_geom(dtype, c, sp, k, s, x_ld=c + pad)
        name = ops.pool_route(g, PASS_FWD, align=align, idx_align=idx_align)
        _check(name, "pool", PASS_FWD, dtype, c, (c + pad, c), align, idx_align)
        lanes = c // _vec(name)               # the line-contiguous kernel merges the two kw lanes of a voxel inside a wave
        assert name.startswith("maxpool2_fwd") == (k == 2 and all(i % 2 == 0 for i in sp) and _vec(name) >= 4 and lanes <= 32 and lanes & (lanes - 1) == 0)
        seen.add(name)
        g = pool_geom(dtype, c, sp, k, s, x_ld=c, y_ld=c + pad)                               # (the gradient passes: dx is dense)
        for addend_ld in (0, c, c + 4):
            name = ops.pool_route(g, PASS_DGRAD, addend_ld=addend_ld, align=align, idx_align=idx_align)
            _check(name, "pool", PASS_DGRAD, dtype, c, (c + pad, c, addend_ld or c), align, idx_align)
            assert name.endswith("+add") == (addend_ld != 0)
            seen.add(name)
    assert seen == {n for p in (PASS_FWD, PASS_DGRAD) for n in VOCABULARY[("pool", p)] if "<" + dtype in n}


UP_KINDS = (("nearest", None, 2, None), ("nearest", None, 4, None), ("nearest", (9, 11, 13), None, None), ("trilinear", None, 2, False),
            ("trilinear", None, 2, True), ("trilinear", (9, 11, 13), None, False))


@pytest.mark.parametrize("dtype", list(TYPES))
def test_upsample_sweep_stays_in_the_vocabulary(dtype):
    seen = set()
    for c, sp, (mode, size, scale, ac), pad, align in itertools.product(CHANNELS, ((3, 5, 7), (4, 6, 8), (1, 1, 1)), UP_KINDS, (0, 4), ALIGNS):
        for pass_ in (PASS_FWD, PASS_DGRAD):
            g = up_geom(dtype, c, sp, mode, size, scale, ac, y_ld=c + pad)
            name = ops.upsample_route(g, pass_, align=align)
            _check(name, "up", pass_, dtype, c, (c, c + pad), align)
            if name.startswith("upsample2x"):
                assert mode == "trilinear" and scale == 2 and not ac
            if name.startswith("upsample2x_bwd"):
                assert name.startswith("upsample2x_bwd_march") == (c % 16 == 0)
            if name.startswith("upsample_nearest_int_bwd"):
                assert mode == "nearest" and name.endswith(",%d>" % scale)
            seen.add(name)
    assert seen == {n for p in (PASS_FWD, PASS_DGRAD) for n in VOCABULARY[("up", p)] if "<" + dtype in n}


# ---- d.
def test_the_segment_length_steps_of_the_x2_forward_keep_their_kernel():
    """One 4 x 16 coarse column of 16 channels at n = 1, d = 4 is a single item (segments of 4 planes); decoder levels of a full-size
    volume (32 and 16 channels at 2 x 40x48x40 and 2 x 80x96x80 coarse) fill the chip with segments of 16.  The segment length is a
    run-time argument, so a name pins the kernel only."""
    assert ops.upsample_route(up_geom("f32", 16, (4, 4, 16), "trilinear", scale=2, ac=False, n=1), PASS_FWD) == "upsample2x_fwd_march<f32,4,4>"
    for c, sp in ((32, (40, 48, 40)), (16, (80, 96, 80))):
        for dtype, fwd in (("f32", "upsample2x_fwd_march<f32,4,%d>" % min(8, c // 4)), ("bf16", "upsample2x_fwd_march<bf16,8,%d>" % (c // 8))):
            assert ops.upsample_route(up_geom(dtype, c, sp, "trilinear", scale=2, ac=False), PASS_FWD) == fwd
            assert ops.upsample_route(up_geom(dtype, c, sp, "trilinear", scale=2, ac=False), PASS_DGRAD) == "upsample2x_bwd_march<%s>" % dtype


# ---- e.
def test_every_parity_row_reaches_the_names_and_numbers_it_declares():
    wrong = [w for r, dtype in rc.PARITY_PAIRS for w in run.declared_mismatches(r, dtype, run.plans(r, dtype))]
    assert not wrong, "%d declaration(s) missed:\n  %s" % (len(wrong), "\n  ".join(wrong))


def _slab_extent(row, pass_, name):
    """(slabs, H extent) of a slab kernel's pass: the forward walks output planes (the line-contiguous pool: output rows of input
    columns), the backward input planes"""
    out = run.out_size(row)
    d, h = (out[0], out[1]) if pass_ == "fwd" else (row.sp[0], row.sp[1])
    return rc.N * d, h


def corner(row, dtype, pass_, name, plan):
    """the plan corner a pass sits in: (kernel, channels per lane item, segment-length class, more work than workgroups, slabs that
    are parts of a plane).  The storage type, the pieces per voxel and the addend select an instantiation or an argument, not another
    plan: b. holds every instantiation to a row."""
    kernel = name[:name.index("<")]
    if name.startswith("upsample2x"):
        return (kernel, plan["vec"], plan["segl"], plan["items"] > plan["grid"], False)
    nd, h = _slab_extent(row, pass_, name)
    hchunks = -(-h // plan["hch"])
    return (kernel, plan["vec"], 0, nd * hchunks > plan["grid"], plan["hch"] < h)


def _corners_of_rows():
    return {corner(r, t, p, *run.plans(r, t)[p]) for r, t in rc.PARITY_PAIRS for p in ("fwd", "bwd")}


def test_the_sections_of_the_parity_table_are_what_they_say():
    def all_(rows, pass_, pred, dtypes=None):
        for r in rows:
            for t in r.dtypes:
                name, plan = run.plans(r, t)[pass_]
                assert pred(corner(r, t, pass_, name, plan)), (r.id, t, pass_, name, plan)
    all_(rc.PARITY_UP_SEGMENTS[:1], "fwd", lambda c: c[2] == 16)
    all_(rc.PARITY_UP_SEGMENTS[1:], "fwd", lambda c: c[2] == 8)
    all_(rc.PARITY_UP_SEGMENTS, "bwd", lambda c: c[3])
    all_([r for r in rc.PARITY_UP_LOOPS if "bwd" not in r.id], "fwd", lambda c: c[3])
    all_([r for r in rc.PARITY_UP_LOOPS if r.id.startswith("slab") or "bwd" in r.id], "bwd", lambda c: c[3])
    all_(rc.PARITY_POOL_LOOPS, "fwd", lambda c: c[3])
    all_(rc.PARITY_POOL_LOOPS, "bwd", lambda c: c[3])
    all_(rc.PARITY_POOL_CHUNKS[:1] + rc.PARITY_POOL_CHUNKS[2:] + rc.PARITY_UP_CHUNKS, "fwd", lambda c: c[4])
    all_(rc.PARITY_POOL_CHUNKS + [r for r in rc.PARITY_UP_CHUNKS if "loop" not in r.id], "bwd", lambda c: c[4])
    all_([r for r in rc.PARITY_UP_CHUNKS if "loop" in r.id], "fwd", lambda c: c[3] and c[4])
    # the ragged last part: chunks of 6, 6 and 1 rows in the line-contiguous pool, 12 and 1 in the slab pool
    r = rc.PARITY_POOL_CHUNKS[0]
    assert run.out_size(r)[1] == 13 and run.plans(r, "f32")["fwd"][1]["hch"] == 6
    # the second channel pass of x2_c36 holds one live piece of eight, that of x2_c20 one of four
    for rid, npv in (("x2_c36_one_live_piece", 8), ("x2_c20_two_passes", 4)):
        r = next(r for r in rc.PARITY_UP if r.id == rid)
        for t in r.dtypes:
            plan = run.plans(r, t)["fwd"][1]
            assert (plan["vec"], plan["npv"], plan["passes"]) == (4, npv, 2) and r.c // 4 - npv == 1


# ---- f.
SWEEP_UP = [((3, 5, 7), None), ((4, 6, 8), None), ((1, 1, 1), None), ((2045, 5, 3), None), ((1030, 5, 3), None), ((4200, 1, 2), None),
            ((2, 9, 70), None), ((2, 9, 300), None), ((1025, 1, 513), None), ((12296, 1, 17), None), ((65552, 1, 1), None), ((1026, 5, 1), None)]
SWEEP_MAX_ELEMENTS = 1 << 24      # a corner that only larger volumes reach has no row: its test would not run in seconds
SWEEP_POOL = [(5, 7, 9), (4, 6, 8), (8, 8, 4), (8200, 2, 2), (8200, 2, 3), (2, 26, 80), (2, 26, 81), (2, 14, 300)]


def test_no_plan_corner_of_a_sweep_is_without_a_parity_row():
    have, missing = _corners_of_rows(), set()
    for dtype, c, align in itertools.product(TYPES, CHANNELS, ALIGNS):
        esz = run.ESZ[dtype]
        lay = None if align == 16 else (c + 16 // esz, align // esz)      # a slice at `align` bytes of a wider buffer
        if lay is not None and (lay[1] * esz) % 16 == 0:
            continue
        layout = {} if lay is None else {"x": lay, "dy": lay, "out": lay, "dskip": lay}
        for sp in SWEEP_POOL:
            for (k, s), addend in itertools.product(((2, 2), (4, 2)), (False, True)):
                row = rc._pool("sweep", c, sp, k=k, s=s, addend=addend, layout=layout, fwd=("", 0, 0), bwd=(0, 0))
                if min(run.out_size(row)) <= 0:
                    continue
                got = run.plans(row, dtype)
                missing |= {corner(row, dtype, p, *got[p]) for p in ("fwd", "bwd")} - have
        for (sp, _), (mode, size, scale, ac) in itertools.product(SWEEP_UP, UP_KINDS):
            if size is not None:
                size = tuple(i + i // 2 + 1 for i in sp)
            row = rc._up("sweep", mode, c, sp, size=size, scale=scale, ac=ac, layout=layout, fwd="%s", bwd="%s")
            if rc.N * c * run.out_size(row)[0] * run.out_size(row)[1] * run.out_size(row)[2] > SWEEP_MAX_ELEMENTS:
                continue
            got = run.plans(row, dtype)
            missing |= {corner(row, dtype, p, *got[p]) for p in ("fwd", "bwd")} - have
    assert not missing, "%d plan corner(s) without a parity row:\n  %s" % (len(missing), "\n  ".join(map(str, sorted(missing))))


# ---- g.
def test_geometries_past_the_32_bit_limits_decline():
    # a fine plane above 2^31 - 1 elements
    sp = (2, 16400, 16400)
    assert 4 * sp[1] * sp[2] * 16 > 2 ** 31 - 1
    g = up_geom("f32", 16, sp, "trilinear", scale=2, ac=False, n=1)
    assert ops.upsample_route(g, PASS_FWD) == "upsample_fwd<f32,4>" and ops.upsample_route(g, PASS_DGRAD) == "upsample2x_bwd<f32>"
    assert ops.upsample_plan(g, PASS_FWD)["items"] == 0 and ops.upsample_plan(g, PASS_DGRAD)["lds_bytes"] > 0
    # more than 0x7ffffff0 items (the plane limits hold: 4 x 2 voxels of 16 channels)
    g = up_geom("f32", 128, (2 ** 27, 8, 1), "trilinear", scale=2, ac=False, n=8)      # 2^31 marching items, 2^30 tiles
    assert ops.upsample_route(g, PASS_DGRAD) == "upsample2x_bwd<f32>" and ops.upsample_plan(g, PASS_DGRAD)["items"] == 2 ** 30
    g = up_geom("f32", 4, (2 ** 29, 1, 1), "trilinear", scale=2, ac=False, n=128)
    assert 128 * 2 ** 29 // 16 > 0x7ffffff0 and ops.upsample_route(g, PASS_FWD) == "upsample_fwd<f32,4>"
    # one sample of 2^31 elements leaves the line-contiguous pool; one element less keeps it
    assert ops.pool_route(pool_geom("f32", 16, (2 ** 9, 2 ** 9, 2 ** 9), 2, 2), PASS_FWD) == "maxpool_fwd<f32,4>"
    assert ops.pool_route(pool_geom("f32", 16, (2 ** 9, 2 ** 9, 2 ** 9 - 2), 2, 2), PASS_FWD) == "maxpool2_fwd<f32,4>"
