"""CPU suite that keeps the fused-convolution parity suite (tests/test_fusedconv_parity_gpu.py) honest without a device:
  a. the float64 reference tests/fusedconv_ref.py agrees with torch's float64 F.conv3d(F.interpolate(..)) and with autograd through
     the two convolutions of the pair, to 1e-13 relative to L1, on the small rows;
  b. every row of tests/fusedconv_cases.py reaches the plan numbers it declares (host-only queries), every (Ci, Co, taps) instance
     is swept at both scales, and the corner rows have the property they are named for;
  c. an fp32 emulation of every pass in the kernel's summation order (tests/fusedconv_emu.py) stays inside the counted bounds;
  d. each deliberate error in that emulation leaves the bounds on rows the GPU module runs."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fusedconv_cases as fc
import fusedconv_emu as emu
import fusedconv_ref as fr
import fusedconv_run as run

REL = 1e-13
BY_ID = {r.id: r for r in fc.UP_ROWS + fc.PAIR_ROWS}
LARGE = ("fwd-slabs-over-grid", "fwd-slabs-over-grid-hch1", "dgrad-rows-over-grid-wc1", "wo-over-1024", "rows-over-grid")
SMALL_UP = [r for r in fc.UP_ROWS if r.id not in LARGE]
SMALL_PAIR = [r for r in fc.PAIR_ROWS if r.id not in LARGE]


def _close(name, got, want, l1):
    err = (got - want).abs()
    assert bool((err <= REL * l1 + 1e-300).all()), "%s: |torch - reference| up to %.3g of L1" % (name, float((err / l1.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("row", SMALL_UP, ids=[r.id for r in SMALL_UP])
def test_upconv_reference_is_torch_float64(row):
    inp = run.make_inputs(row, "f32")
    ref = run.reference(row, inp)
    x = inp["x"].double().requires_grad_(True)
    w = inp["w"].double().requires_grad_(True)
    b = inp["b"].double().requires_grad_(True) if inp["b"] is not None else None
    y = F.conv3d(F.interpolate(x, scale_factor=row.S, mode="nearest"), w, b, padding=row.pad)
    y.backward(inp["dy"].double())
    _close("y", y.detach(), ref["y"][0], ref["y"][1])
    _close("dx", x.grad, ref["dx"][0], ref["dx"][1])
    _close("dw", w.grad, ref["dw"][0], ref["dw"][1])
    dbias = inp["dy"].double().sum(dim=(0, 2, 3, 4)) if b is None else b.grad
    _close("dbias", dbias, ref["dbias"][0], ref["dbias"][1])
    # the term counts: every tap in range contributes Ci (forward) terms; an interior voxel of a 'same' layer has them all
    taps = row.k[0] * row.k[1] * row.k[2]
    assert float(ref["y"][2].max()) <= taps * row.ci + 1 and float(ref["dx"][2].max()) <= taps * row.co * row.S ** 3


@pytest.mark.parametrize("row", SMALL_PAIR, ids=[r.id for r in SMALL_PAIR])
def test_pair_reference_is_autograd_of_the_two_convolutions(row):
    inp = run.make_inputs(row, "f32")
    ref = run.reference(row, inp)
    g = torch.Generator().manual_seed(5)
    w1 = torch.randn((run.C, 1, run.K1, 1, 1), generator=g, dtype=torch.float64).requires_grad_(True)
    b1 = torch.randn(run.C, generator=g, dtype=torch.float64).requires_grad_(True)
    a1 = F.conv3d(inp["x"].double(), w1, b1, stride=(row.s1, 1, 1), padding=(row.p1, 0, 0))
    y2 = F.conv3d(a1, inp["w2"].double(), None, stride=(1, row.s2, 1), padding=(0, row.p2, 0))
    assert tuple(y2.shape) == tuple(inp["dy2"].shape)
    y2.backward(inp["dy2"].double())
    _close("dw1", w1.grad, ref["dw1"][0], ref["dw1"][1])
    _close("dbias1", b1.grad, ref["dbias1"][0], ref["dbias1"][1])


def test_rows_reach_their_declared_plans_and_cover_every_instance():
    wrong = []
    for row, dtype in fc.UP_PAIRS + fc.PAIR_PAIRS:
        wrong += run.declared_mismatches(row, dtype, run.plans(row, dtype))
    assert not wrong, "\n".join(wrong)
    # the instances the sweep names are those upconv.hip compiles: a new one needs its rows
    src = open(os.path.join(os.path.dirname(run.ops.__file__), "csrc", "upconv.hip")).read()
    macro = re.search(r"#define MRI3D_UPCONV_INSTANCES\(X\)((?:.*\\\n)*.*)\n", src).group(1)
    assert [tuple(map(int, m)) for m in re.findall(r"X\((\d+), (\d+), (\d+)\)", macro)] == fc.INSTANCES
    p = run.plans(BY_ID["fwd-slabs-over-grid-hch1"], "f32")["fwd"]
    assert p["hch"] == 1 and p["slabs"] > 4096 and p["slabs"] % p["grid"]
    swept = {(r.ci, r.co, r.k[0] * r.k[1] * r.k[2], r.S) for r in fc.UP_SWEEP}
    assert swept == {(ci, co, t, S) for ci, co, t in fc.INSTANCES for S in (2, 4)}
    for S in (2, 4):                                     # every axis carries taps of a 3- and of a 6-tap instance at every scale
        for t in (3, 6):
            axes = {a for r in fc.UP_SWEEP if r.S == S and r.k[0] * r.k[1] * r.k[2] == t for a in range(3) if r.k[a] > 1}
            assert axes == {0, 1, 2}, (S, t, axes)
    assert any(r.k == (2, 3, 1) for r in fc.UP_SWEEP) and any(r.k == (1, 3, 2) for r in fc.UP_SWEEP)
    assert any(max(r.k) == 3 and max(r.pad) == 2 for r in fc.UP_SWEEP) and any(r.k == (1, 1, 1) and r.pad == (1, 1, 1) for r in fc.UP_SWEEP)
    # the properties the corner rows are named for, from the queried numbers
    p = run.plans(BY_ID["fwd-slabs-over-grid"], "f32")
    assert p["fwd"]["slabs"] > 4096 and p["fwd"]["slabs"] % p["fwd"]["grid"] and p["wgrad"]["slabs"] > 1024 and p["wgrad"]["slabs"] % 1024
    assert p["fwd"]["hch"] * run.up_extents(BY_ID["fwd-slabs-over-grid"])[1][2] < 256               # inner < 256
    for rid in ("ragged-slab", "ragged-slab-s4"):
        ho = run.up_extents(BY_ID[rid])[1][1]
        hch = run.plans(BY_ID[rid], "f32")["fwd"]["hch"]
        assert hch < ho and ho % hch
    assert run.up_extents(BY_ID["wo-over-1024"])[1][2] > 1024
    assert run.plans(BY_ID["dgrad-rows-over-grid-wc1"], "f32")["dgrad"]["rows"] > 8192 and BY_ID["dgrad-rows-over-grid-wc1"].sp[2] == 1
    for rid, wc in (("wc5-s4", 5), ("wc33-s2", 33)):
        assert BY_ID[rid].sp[2] == wc == run.plans(BY_ID[rid], "f32")["dgrad"]["per"] + 1
    p = run.plans(BY_ID["rows-over-grid"], "f32")
    assert p["rows"] > 4096 and p["rows"] % 4 and run.plans(BY_ID["rows-under-4"], "f32")["rows"] < 4
    assert {r.sp[2] for r in fc.PAIR_ROWS} >= {1, 63, 64, 65, 130}
    assert {(r.k2, r.s2, r.p2) for r in fc.PAIR_ROWS} >= {(6, 2, 2), (3, 1, 1), (6, 3, 2), (8, 3, 3), (1, 1, 0), (2, 3, 0), (5, 2, 4), (4, 2, 0)}
    assert {(r.s1, r.p1) for r in fc.PAIR_ROWS} >= {(2, 2), (1, 0), (3, 5), (2, 0)}


# ---------------------------------------------------------------------------------------------- the emulation against the bounds
_cache = {}


def _setup(row, dtype):
    """(inputs as numpy fp32, reference, plan) of a row, computed once"""
    key = (row.id, dtype)
    if key not in _cache:
        inp = run.make_inputs(row, dtype)
        _cache[key] = ({k: (v.float().numpy() if v is not None else None) for k, v in inp.items()}, run.reference(row, inp), run.plans(row, dtype))
    return _cache[key]


def _store(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(run.TORCH[dtype]) if dtype == "bf16" else t


def emulate(row, dtype, passes, err=None):
    """{name: result of the storage type} of the passes named, with the deliberate error `err`"""
    a, _, plan = _setup(row, dtype)
    got = {}
    if not run.is_up(row):
        dw, db = emu.pair_wgrad_first(a["x"], a["dy2"], a["w2"], row.s1, row.p1, row.s2, row.p2, plan, err)
        return {"dw1": torch.from_numpy(dw), "dbias1": torch.from_numpy(db)}
    if "fwd" in passes:
        got["y"] = _store(emu.upconv_fwd(a["x"], a["w"], a["b"], row.S, row.pad, plan["fwd"], err), dtype)
    if "dgrad" in passes:
        got["dx"] = _store(emu.upconv_dgrad(a["dy"], a["w"], row.S, row.pad, row.sp, plan["dgrad"], err), dtype)
    if "wgrad" in passes:
        dw, db = emu.upconv_wgrad(a["x"], a["dy"], row.S, row.pad, row.k, plan["wgrad"], err)
        got.update(dw=torch.from_numpy(np.ascontiguousarray(dw)), dbias=torch.from_numpy(db))
    return got


def worst(row, dtype, got):
    _, ref, plan = _setup(row, dtype)
    return {name: ratio for name, ratio, _ in run.report(row, dtype, ref, plan, got)}


# every row in both storage types; the large rows once, in fp32: the storage type changes no summation order
EMULATED = [(r, d) for r, d in fc.UP_PAIRS + fc.PAIR_PAIRS if d == "f32" or r.id not in LARGE]


@pytest.mark.parametrize("row,dtype", EMULATED, ids=["%s-%s" % (r.id, d) for r, d in EMULATED])
def test_fp32_emulation_in_kernel_order_stays_inside_the_bounds(row, dtype):
    ratios = worst(row, dtype, emulate(row, dtype, ("fwd", "dgrad", "wgrad")))
    assert ratios and max(ratios.values()) <= 1.0, (row.id, dtype, ratios)


SWEEP_IDS = [r.id for r in fc.UP_SWEEP]
PADDED = [r.id for r in fc.UP_SWEEP if max(r.pad) > 0]
DGRAD_PASSES = ["wc5-s4", "wc33-s2", "wc10-s4-three-passes", "wc70-s2-three-passes"]
# (error, pass, result it must spoil, rows): on EVERY row listed the emulation with the error must leave the bound
ERRORS = [
    ("coarse_pad", "fwd", "y", PADDED),
    ("drop_slab", "fwd", "y", ["fwd-slabs-over-grid"]),
    ("tap_sign", "dgrad", "dx", [i for i in SWEEP_IDS if "t1-" not in i]),
    ("skip_xor", "dgrad", "dx", SWEEP_IDS),
    ("c0_stuck", "dgrad", "dx", SWEEP_IDS),
    ("no_live", "dgrad", "dx", DGRAD_PASSES),
    ("drop_slab", "wgrad", "dw", ["fwd-slabs-over-grid", "fwd-slabs-over-grid-hch1"]),
    ("drop_slab", "wgrad", "dbias", ["fwd-slabs-over-grid"]),
    ("drop_ragged", "wgrad", "dw", ["ragged-slab", "ragged-slab-s4"]),
    ("drop_ragged", "wgrad", "dbias", ["ragged-slab", "ragged-slab-s4"]),
    ("kh0", "pair", "dw1", ["k6s2p2-shipped-w65", "k8s3p3-w130", "k5s2p4", "k6s3p2-w64"]),
    ("kh0", "pair", "dbias1", ["k6s2p2-shipped-w65", "k8s3p3-w130", "k5s2p4", "k6s3p2-w64"]),
    ("x_plane", "pair", "dw1", ["k6s2p2-shipped-w65", "first-s3p5"]),
]
FLAG_CASES = [(e, p, name, rid) for e, p, name, rids in ERRORS for rid in rids]


@pytest.mark.parametrize("err,pass_,name,rid", FLAG_CASES, ids=["%s-%s-%s-%s" % c for c in FLAG_CASES])
def test_deliberate_error_leaves_the_bound(err, pass_, name, rid):
    row = BY_ID[rid]
    clean = worst(row, "f32", emulate(row, "f32", (pass_,)))[name]
    spoiled = worst(row, "f32", emulate(row, "f32", (pass_,), err))[name]
    assert clean <= 1.0 < spoiled, "%s on %s: %s clean %.3g, with the error %.3g of the bound" % (err, rid, name, clean, spoiled)
