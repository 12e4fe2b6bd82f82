"""CPU suite: which kernel every convolution parity case runs on, and that every kernel has one.

The route of a convolution (kernel family, kernel, template instantiation) is a host decision that mri3d_conv3d_route answers
without a device, from the same function the entry points launch by.  So the coverage of the GPU parity suite is checked here:

  a. every case of tests/conv_cases.py reaches the route its table declares (`expect`) and its own row of PER_CASE;
  b. every route name the dispatcher can return (MATRIX, hand-written) is reached by a case that is compared with a CPU reference
     through the plain entry points, one of them ragged in d, h and w — or carries the reason why it has none;
  c. a sweep over geometries, dtypes, pitches, strides, statistics and split operands finds no route name outside MATRIX, and
     every name in it;
  d. wherever the dispatcher chooses the marching kernel, the by-name entry points of tests/test_march_gpu.py run the plan it
     launches: the same statistics-block count (= grid) for the forward, mri3d_conv3d_march_supported for the data gradient.

A performance change that moves a threshold fails here, before any GPU time, with the names of the cases that left their kernel
and of the kernels that lost their last case."""
import ctypes

import pytest

import conv_cases as cc
from mri_epilepsy_diagnosis_amd import _lib, ops
from mri_epilepsy_diagnosis_amd._lib import BF16, F32, PASS_DGRAD, PASS_FWD, PASS_WGRAD

# ---- b. every route name, per dtype and pass.  None: a parity case must reach it; a string: why none does.
_F32_MARCH = ("fp32 takes the marching kernel from 4 Mi voxels up only: test_march_gpu.py compares the same kernel and plan by name on small "
              "volumes (check d), test_buffer_contracts_gpu.py's f32_march case samples the full volume against float64")
_DGRAD_BIAS = "only ConvTranspose3d passes a bias to the data gradient, and no model here has a 3x3x3 stride-1 pad-1 one at a marching size"
_DIRECT = ["direct nt%d mode%d split%d" % (nt, m, s) for nt, m, s in ((1, 0, 0), (1, 0, 1), (2, 0, 0), (4, 0, 0))]
_DIRECT_DGRAD_S = ["direct nt%d mode1 split%d" % (nt, s) for nt, s in ((1, 0), (1, 1), (2, 0), (4, 0))]   # stride > 1
_TILED = ["tiled nt1", "tiled nt2", "tiled_n8"]


# conv_generic.hip / conv_pointwise.hip: "<file> <kernel> <template arguments and branches>" (include/mri3d.h)
_TL = (16, 8, 4, 2)
_C1TAPS = ("conv_c1_taps_kernel / conv_c1_taps_wgrad_kernel need W % 4 == 0 (16-byte rows), so no case is ragged in w: a case with odd "
           "d and h above one is required instead")
_GATHER = ["generic gather tl%d vec%d" % (t, v) for t in _TL for v in (0, 1)]
_GEN_FWD = ["generic c1c1", "generic cin1 co8", "generic cin1 co16"] + _GATHER + \
           ["generic taps tl%d nt%d cv4" % (t, n) for t in _TL for n in (3, 4, 6, 8)] + ["generic taps tl%d nt%d cv1" % (t, n) for t in _TL for n in (3, 6, 8)] + \
           ["pointwise co2", "pointwise co4"]
_GEN_DGRAD = ["generic c1c1"] + _GATHER + ["generic strided tl%d vec%d" % (t, v) for t in _TL for v in (0, 1)] + \
             ["generic staps tl%d nt%d" % (t, n) for t in _TL for n in (3, 4, 8)] + \
             ["generic taps tl%d nt%d cv4" % (t, n) for t in _TL for n in (3, 4, 6, 8)] + ["generic taps tl%d nt%d cv1" % (t, n) for t in _TL for n in (3, 8)] + \
             ["pointwise co2", "pointwise co4", "pointwise co8"]
_GEN_WGRAD = ["generic c1c1", "generic cin1 co8", "generic cin1 co16", "generic small", "generic lds", "generic quads nt8 civ1"] + \
             ["generic co1 ci%d" % c for c in (1, 4, 8, 16)] + ["generic quads nt%d civ4" % n for n in (4, 6, 8)] + \
             ["pointwise co%d vx4 dv%d" % (c, v) for c in (2, 4, 8) for v in (0, 1)]
_PW_WGRAD_BF16 = ["pointwise co%d vx8 dv%d" % (c, v) for c in (2, 4) for v in (0, 1)]       # 16-byte bf16 loads: 8 channels per lane
_C1TAPS_NAMES = ["generic c1taps nt3", "generic c1taps nt8"]                                # fp32 only: no bf16 instantiation exists


def _with_bias(names):
    """a data gradient that adds a bias is the forward of a ConvTranspose3d (cases: the TRANSPOSE table)"""
    return list(names) + [n + " bias" for n in names]


def _own_file(name):
    return name.split(" ")[0] in ("generic", "pointwise")


def _entries(covered, uncovered=()):
    out = {name: None for name in covered}
    out.update(dict(uncovered))
    return out


MATRIX = {
    ("f32", "fwd"): _entries(_GEN_FWD + _DIRECT + _TILED, [("march", _F32_MARCH), ("march bias", _F32_MARCH)] + [(n, _C1TAPS) for n in _C1TAPS_NAMES]),
    ("f32", "stats"): _entries(["tiled nt1 stats", "tiled nt2 stats"], [("march stats", _F32_MARCH), ("march stats bias", _F32_MARCH)]),
    ("f32", "dgrad"): _entries(_with_bias(_GEN_DGRAD) + _DIRECT + _DIRECT_DGRAD_S + _TILED,
                               [("march", _F32_MARCH), ("march bias", _DGRAD_BIAS)] + [(n, _C1TAPS) for n in _with_bias(_C1TAPS_NAMES)]),
    ("f32", "wgrad"): _entries(_GEN_WGRAD + ["cin1", "wgrad3", "wgrad6", "wgrad6 co8", "wgrad6 ci8 co8"], [(n, _C1TAPS) for n in _C1TAPS_NAMES]),
    # bf16 tensors take the LDS-free kernel only with a stride
    ("bf16", "fwd"): _entries(_GEN_FWD + ["march", "march bias"] + _DIRECT + _TILED),
    ("bf16", "stats"): _entries(["tiled nt1 stats", "tiled nt2 stats", "march stats", "march stats bias"]),
    ("bf16", "dgrad"): _entries(_with_bias(_GEN_DGRAD) + ["march"] + _DIRECT_DGRAD_S + _TILED, [("march bias", _DGRAD_BIAS)]),
    ("bf16", "wgrad"): _entries(_GEN_WGRAD + _PW_WGRAD_BF16 + ["cin1", "wgrad3", "wgrad4", "bf16", "bf16t"]),
}


# ---- a.
@pytest.mark.parametrize("table", list(cc.TABLES.values()), ids=lambda t: t.name)
def test_every_case_reaches_the_route_its_table_declares(table):
    wrong = []
    for case, dtype in cc.pairs(table):
        try:
            table.check(case, dtype)
        except AssertionError as e:
            wrong.append(str(e))
    assert not wrong, "%d case(s) left their kernel:\n  %s" % (len(wrong), "\n  ".join(wrong))


def test_per_case_rows_belong_to_cases():
    """No row of PER_CASE without its case (a renamed or removed case must take its row along)."""
    for (name, dtype), rows in cc.PER_CASE.items():
        table = cc.TABLES[name]
        ids = {table.ids(c) for c, dt in cc.pairs(table) if dt == dtype}
        assert set(rows) == ids, (name, dtype, sorted(set(rows) ^ ids))


# ---- b.
def _covered():
    """{(dtype, pass): {route name: [(table, case id, ragged)]}} over the tables whose tests compare with a CPU reference."""
    out = {}
    for table, case, dtype in cc.all_pairs():
        if not table.oracle:
            continue
        for p, name in table.routes(case, dtype).items():
            shape = table.shape(case, p)
            p = cc.KERNEL_PASS.get(table.kind, {}).get(p, p)       # (a transposed convolution runs the mirrored one's passes)
            out.setdefault((dtype, p), {}).setdefault(name, []).append((table.name, table.ids(case), cc.is_ragged(*shape), shape))
    return out


def test_every_route_has_a_parity_case_and_a_ragged_one():
    covered = _covered()
    missing, stale = [], []
    for key, names in MATRIX.items():
        for name, reason in names.items():
            cases = covered.get(key, {}).get(name, [])
            if reason is None:
                if not cases:
                    missing.append("%s %s '%s': no parity case" % (key + (name,)))
                elif not any(c[2] for c in cases):
                    missing.append("%s %s '%s': no case ragged in d, h and w (has %s)" % (key + (name, ", ".join("%s %s" % c[:2] for c in cases[:3]))))
            elif reason is _C1TAPS:
                if not any(d > 1 and h > 1 and d % 2 == 1 and h % 2 == 1 for _, _, _, (_, d, h, _) in cases):
                    missing.append("%s %s '%s': no case with odd d and h" % (key + (name,)))
            else:
                assert len(reason) > 20, (key, name)
                if cases:
                    stale.append("%s %s '%s' is reached by %s %s: drop its reason" % (key + (name,) + cases[0][:2]))
    assert not missing, "kernels without an operator-level oracle case:\n  " + "\n  ".join(missing)
    assert not stale, "\n".join(stale)
    for key, names in covered.items():
        assert set(names) <= set(MATRIX[key]), (key, sorted(set(names) - set(MATRIX[key])))


# ---- c. / d.
_CH = [1, 3, 4, 8, 12, 16, 20, 24, 32, 40, 48, 64, 96, 128]
_VOLUMES = [(1, 1, 1, 1), (1, 2, 3, 5), (2, 5, 9, 17), (1, 8, 8, 8), (300, 8, 8, 8), (64, 5, 9, 17), (40, 5, 9, 19), (3, 17, 40, 65), (1, 40, 48, 40),
            (8, 45, 17, 37), (1, 200, 100, 60), (2, 160, 192, 160), (300, 3, 7, 21), (64, 41, 12, 20), (48, 41, 5, 9)]
_PADS = [(0, 0), (4, 0), (0, 4), (8, 8), (16, 0), (0, 16)]
_PASSES = ((PASS_FWD, "fwd"), (PASS_DGRAD, "dgrad"), (PASS_WGRAD, "wgrad"))


def _filters():
    """(kernel, stride, padding, dilation) beyond 3x3x3 / pad 1: what conv_generic.hip and conv_pointwise.hip choose their kernels by."""
    one, zero = (1, 1, 1), (0, 0, 0)
    for k in (2, 3, 4, 5, 6):                       # separable filters along each axis, stride 1 and 2 (the autoencoder's blocks)
        for ax in range(3):
            for s in (1, 2):
                kk, ss, pp = [1, 1, 1], [1, 1, 1], [0, 0, 0]
                kk[ax], ss[ax], pp[ax] = k, s, (k // 2 if s == 1 else (k - 1) // 2)
                yield tuple(kk), tuple(ss), tuple(pp), one
    yield (2, 2, 2), one, zero, one
    yield (2, 2, 2), (2, 2, 2), zero, one
    yield (1, 2, 2), one, (0, 1, 1), one            # exactly four taps
    yield (3, 3, 1), (2, 2, 1), (1, 1, 0), one      # four valid taps per input voxel in the strided data gradient
    yield (4, 4, 4), (4, 4, 4), zero, one
    yield (4, 4, 4), (2, 2, 2), one, one            # (the mirrored convolution of ConvTranspose3d(k 4, s 2, p 1); output padding only changes extents)
    yield (3, 3, 3), (2, 2, 2), one, one
    yield (3, 3, 3), one, (2, 2, 2), (2, 2, 2)
    yield (3, 3, 3), one, (3, 3, 3), (3, 3, 3)
    yield (3, 3, 3), (2, 2, 2), zero, (3, 3, 3)
    for st in ((2, 1, 1), (1, 2, 1), (1, 1, 2)):
        yield (3, 3, 3), st, one, one
    yield (5, 5, 5), one, (2, 2, 2), one


_CH_GENERIC = [1, 2, 3, 4, 5, 8, 16, 32, 64]            # (2: the classifier's 16 -> 2, the only way to the one-load dy of two channels)
_VOL_GENERIC = [(1, 7, 9, 11), (2, 8, 12, 16)]            # the new filters on a ragged volume and one whose W is a multiple of 4
_PITCH_GENERIC = [(0, 0), (4, 4), (1, 1), (4, 1), (1, 4)]
_ALIGNS = [(ax, ay) for ax in (16, 8, 4) for ay in (16, 8, 4)]


def _generic_geoms():
    """(dtype name, geometry) of the filters above (and 3x3x3 / pad 1, 1x1x1) over channels 1-64 and pitches +0 / +4 / +1."""
    one, zero = (1, 1, 1), (0, 0, 0)
    for dn, dt in cc.DTYPES.items():
        for k, s, p, dil in list(_filters()) + [((3, 3, 3), one, one, one), (one, one, zero, one)]:
            for ci in _CH_GENERIC:
                for co in _CH_GENERIC:
                    for vi, (n, d, h, w) in enumerate(_VOL_GENERIC):
                        for pi, po in (_PITCH_GENERIC if vi == 0 else _PITCH_GENERIC[:1]):
                            yield dn, ops._conv_geom((n, ci, d, h, w), (co, ci) + k, s, p, dil, x_ld=ci + pi, y_ld=co + po, dtype=dt)


def _geoms():
    """(dtype name, geometry, may take a split) over channels 1-128, extents 1-200, batches 1-300, pitches +0/4/8/16, strides 1-3 of
    the 3x3x3 / pad 1 convolution, and the 1x1x1 one."""
    one = (1, 1, 1)
    for dn, dt in cc.DTYPES.items():
        for ci in _CH:
            for co in _CH:
                for n, d, h, w in _VOLUMES:
                    for s in (1, 2, 3):
                        for pi, po in (_PADS if s == 1 else _PADS[:1] + _PADS[3:4]):
                            yield dn, ops._conv_geom((n, ci, d, h, w), (co, ci, 3, 3, 3), (s,) * 3, one, one, x_ld=ci + pi, y_ld=co + po, dtype=dt), s == 1 and ci >= 32
                    yield dn, ops._conv_geom((n, ci, d, h, w), (co, ci, 1, 1, 1), one, (0, 0, 0), one, dtype=dt), False


@pytest.fixture(scope="module")
def sweep():
    """{(dtype, pass): set of names} of the plain entry points, the same of the *_cat entry points, and the geometries sent to the
    marching kernel: [(dtype, geometry, pass name)]."""
    L = _lib.lib()
    name = ctypes.create_string_buffer(64)
    plain, split, marched = {}, {}, []

    def route(g, p, stats, bias, sp=0, ld=0, align=16, align_y=None):
        rc = L.mri3d_conv3d_route(ctypes.byref(g), p, stats, bias, sp, ld, align, align if align_y is None else align_y, name, 64)
        assert rc == 0, L.mri3d_last_error()
        return name.value.decode()

    for dn, g, splittable in _geoms():
        for p, pn in _PASSES:
            for bias in ((0, 1) if p != PASS_WGRAD else (0,)):
                r = route(g, p, 0, bias)
                plain.setdefault((dn, pn), set()).add(r)
                if r == "march":
                    marched.append((dn, g, pn))
            if splittable:
                for ld in (g.ci - 16, g.ci - 12):
                    split.setdefault((dn, pn), set()).add(route(g, p, 0, 1, 16, ld))
        for bias in (0, 1):
            plain.setdefault((dn, "stats"), set()).add(route(g, PASS_FWD, 1, bias))
        if splittable:
            split.setdefault((dn, "stats"), set()).add(route(g, PASS_FWD, 1, 1, 16, g.ci - 16))
        # a misaligned tensor never reaches the kernels that move 16-byte pieces
        assert _own_file(route(g, PASS_FWD, 0, 1, align=4))
    # the kernels of conv_generic.hip / conv_pointwise.hip: both tensors' alignments independently; a tensor that is not aligned to
    # four elements never reaches an instantiation that loads it in vectors
    x_vec = {PASS_FWD: ("cv4", "vec1"), PASS_DGRAD: (), PASS_WGRAD: ("civ4", "vx8", "co1 ci4", "co1 ci8", "co1 ci16")}
    y_vec = {PASS_FWD: (), PASS_DGRAD: ("cv4", "vec1", "staps"), PASS_WGRAD: ("civ4", "cin1", "dv1")}
    for dn, g in _generic_geoms():
        for p, pn in _PASSES:
            for ax, ay in _ALIGNS:
                for bias in ((0, 1) if p == PASS_DGRAD else (0,)):
                    r = route(g, p, 0, bias, align=ax, align_y=ay)
                    plain.setdefault((dn, pn), set()).add(r)
                    if _own_file(r):
                        words = r.split(" ", 1)[1]
                        assert ax > 4 or not any(v in words for v in x_vec[p]), (dn, pn, ax, ay, r)
                        assert ay > 4 or not any(v in words for v in y_vec[p]), (dn, pn, ax, ay, r)
                    else:
                        assert ax == 16 and ay == 16, (dn, pn, ax, ay, r)      # the MFMA kernels move both in 16-byte pieces
    return plain, split, marched


def test_the_dispatcher_returns_no_route_outside_the_matrix(sweep):
    plain, split, _ = sweep
    for key, names in MATRIX.items():
        found = plain[key] - {"none"}
        assert found == set(names), "%s %s: the sweep found %s outside the matrix and did not find %s — a new kernel or instantiation goes into MATRIX " \
                                    "(and gets a parity case), a removed one leaves it" % (key + (sorted(found - set(names)), sorted(set(names) - found)))
        # the *_cat entry points launch kernels of the same vocabulary, or refuse
        assert split[key] - {"none"} <= {n for n in names if not _own_file(n)}, (key, sorted(split[key]))
    assert "none" not in plain[("f32", "fwd")] | plain[("f32", "dgrad")] | plain[("f32", "wgrad")]     # only statistics and splits can be refused
    assert "none" in plain[("f32", "stats")] and "none" in split[("bf16", "wgrad")]


def _march_plan_is_the_by_name_plan(dn, g, pn):
    L = _lib.lib()
    what = (dn, pn, g.n, g.ci, g.co, g.di, g.hi, g.wi, g.x_ld, g.y_ld)
    if pn == "dgrad":
        assert L.mri3d_conv3d_march_supported(ctypes.byref(g), PASS_DGRAD) == 1, what
        return
    blocks = L.mri3d_conv3d_fwd_stats_blocks(ctypes.byref(g))
    assert blocks > 0 and blocks == L.mri3d_conv3d_march_stats_blocks(ctypes.byref(g)), what
    assert L.mri3d_conv3d_march_supported(ctypes.byref(g), PASS_FWD) == 1, what
    assert ops.conv_route(g, PASS_FWD, True, False) == "march stats", what


def test_march_by_choice_is_the_plan_the_by_name_entry_points_run(sweep):
    marched = sweep[2]
    assert len(marched) > 100 and {(dn, pn) for dn, _, pn in marched} == {(dn, pn) for dn in ("f32", "bf16") for pn in ("fwd", "dgrad")}
    for dn, g, pn in marched:
        _march_plan_is_the_by_name_plan(dn, g, pn)


# the layers of the benchmark's U-Net (2 x 160x192x160 at full resolution, 80x96x80 below) that run on the marching kernel
BENCH_MARCH = [("f32", 16, 16, 0, "fwd"), ("f32", 16, 16, 0, "dgrad"), ("f32", 8, 16, 0, "fwd"), ("f32", 48, 16, 0, "dgrad"), ("f32", 16, 32, 0, "dgrad"),
               ("f32", 16, 8, 0, "dgrad")] + \
              [("bf16", ci, co, 0, "fwd") for ci, co in ((8, 8), (8, 16), (16, 16), (48, 16), (24, 8), (16, 8))] + \
              [("bf16", ci, co, 0, "dgrad") for ci, co in ((8, 8), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (48, 16), (24, 8), (16, 8))] + \
              [("bf16", 32, 32, 1, "dgrad"), ("bf16", 32, 64, 1, "dgrad"), ("bf16", 48, 16, 1, "dgrad"), ("bf16", 24, 8, 1, "dgrad")]


@pytest.mark.parametrize("layer", BENCH_MARCH, ids=lambda l: "%s_%d-%d_level%d_%s" % l)
def test_benchmark_layers_on_the_marching_kernel(layer):
    dn, ci, co, level, pn = layer
    vol = (160 >> level, 192 >> level, 160 >> level)
    one = (1, 1, 1)
    g = ops._conv_geom((2, ci) + vol, (co, ci, 3, 3, 3), one, one, one, dtype=cc.DTYPES[dn])
    r = ops.conv_route(g, PASS_FWD if pn == "fwd" else PASS_DGRAD, False, False)
    assert r == "march", (layer, r)
    _march_plan_is_the_by_name_plan(dn, g, pn)


def test_route_query_follows_the_alignment_of_the_real_pointers():
    """`ops._ptr_align` feeds the query what the entry points compute from the pointers: a slice 8 bytes into a buffer is no MFMA
    operand; the bf16 pointwise kernels still take it (4 elements = 8 bytes)."""
    import torch
    buf = torch.zeros(1, 20, 2, 3, 5).contiguous(memory_format=torch.channels_last_3d)
    base = ops._ptr_align(buf)
    assert base == 16
    assert ops._ptr_align(buf[:, 2:]) == 8 and ops._ptr_align(buf[:, 1:]) == 4 and ops._ptr_align(buf, buf[:, 2:]) == 8
    assert ops._ptr_align(None, buf) == 16
    one = (1, 1, 1)
    g = ops._conv_geom((1, 16, 5, 9, 17), (16, 16, 3, 3, 3), one, one, one, x_ld=20, dtype=F32)
    assert ops.conv_route(g, PASS_FWD, align=16).startswith("direct") and ops.conv_route(g, PASS_FWD, align=8) == "generic gather tl16 vec0"
    # the two tensors of a pass are told apart: a misaligned y keeps x's vector loads, and takes the MFMA kernels away just the same
    assert ops.conv_route(g, PASS_FWD, x_align=16, y_align=8) == "generic gather tl16 vec1"
    pw = ops._conv_geom((1, 16, 5, 9, 17), (2, 16, 1, 1, 1), one, (0, 0, 0), one, x_ld=20, dtype=BF16)
    assert ops.conv_route(pw, PASS_FWD, align=8) == "pointwise co2" and ops.conv_route(pw, PASS_FWD, align=4) == "generic gather tl2 vec0"
    # the pointwise kernels only need their x-side tensor aligned: x in the forward and the weight gradient, dx in the data gradient
    assert ops.conv_route(pw, PASS_DGRAD, x_align=16, y_align=2) == "pointwise co2" and ops.conv_route(pw, PASS_DGRAD, x_align=4, y_align=16).startswith("generic ")
    sep = ops._conv_geom((1, 8, 5, 9, 17), (8, 8, 3, 1, 1), one, (1, 0, 0), one, dtype=F32)
    assert ops.conv_route(sep, PASS_WGRAD) == "generic quads nt4 civ4" and ops.conv_route(sep, PASS_WGRAD, x_align=8, y_align=16) == "generic small"
    with pytest.raises(_lib.Mri3dError):
        ops.conv_route(g, PASS_WGRAD, stats=True)
