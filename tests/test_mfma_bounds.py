"""CPU suite that keeps the bounds of the MFMA-family parity suite honest (tests/mfma_ref.py; tests/test_mfma_parity_gpu.py): the
float64 reference agrees with torch's float64 convolution, its autograd and torch.nn.grad.conv3d_weight; an fp32 emulation of each
pass in the kernel's own order of summation (tests/mfma_emu.py) stays inside the bounds on every row small enough to emulate; and
each of ten deliberate errors — the ones these kernels' corners can make — leaves the bounds on the rows named here, in both
storage types where it applies."""
import pytest
import torch
import torch.nn.functional as F

import mfma_cases as mc
import mfma_emu as emu
import mfma_ref as ref
import mfma_run as run

ROWS = {r.id: r for r in mc.ROWS}


@pytest.mark.parametrize("rid,dtype", [("tile-ragged-5x9x17", "f32"), ("kc24", "bf16"), ("tile-1x1x1", "bf16"), ("s2-odd-extents-kc12", "f32"),
                                       ("s3-kc20", "bf16"), ("stats-n3", "bf16")])
def test_reference_agrees_with_torchs_float64_operators(rid, dtype):
    row = ROWS[rid]
    inp = run.make_inputs(row, dtype)
    s = row.stride
    x, dy, w = inp["x"].double(), inp["dy"].double(), ref.stored_weights(inp["w"], dtype, "tiled")
    b = inp["b"].double() if inp["b"] is not None else None
    y, A, a, A0 = ref.forward(x, w, b, s)
    assert torch.equal(y, F.conv3d(x, w, b, stride=s, padding=1)) or (y - F.conv3d(x, w, b, stride=s, padding=1)).abs().max() <= 1e-12 * A.max()
    assert (A - F.conv3d(x.abs(), w.abs(), b.abs() if b is not None else None, stride=s, padding=1)).abs().max() <= 1e-12 * A.max()
    assert torch.equal(a, F.conv3d(x, w, None, stride=s, padding=1)) and tuple(y.shape[2:]) == run.out_sp(row)
    opad = tuple(e - 1 - (o - 1) * s for e, o in zip(row.sp, run.out_sp(row)))          # what conv_transpose3d must add to reach the input
    dx, L1 = ref.dgrad(dy, w, x.shape, s)
    assert (dx - F.conv_transpose3d(dy, w, None, stride=s, padding=1, output_padding=opad)).abs().max() <= 1e-12 * L1.max()
    assert (L1 - F.conv_transpose3d(dy.abs(), w.abs(), None, stride=s, padding=1, output_padding=opad)).abs().max() <= 1e-12 * L1.max()
    xg = x.clone().requires_grad_(True)
    F.conv3d(xg, w, None, stride=s, padding=1).backward(dy)
    assert (dx - xg.grad).abs().max() <= 1e-12 * L1.max()
    if dtype == "bf16":
        assert torch.equal(w, inp["w"].to(torch.bfloat16).double()) and not torch.equal(w, inp["w"].double())
        assert torch.equal(ref.stored_weights(inp["w"], dtype, "direct"), inp["w"].double())
    if s == 1:
        dw, L1w, db, L1b = ref.wgrad(x, dy, row.co)
        want = torch.nn.grad.conv3d_weight(x, w.shape, dy, padding=1)
        assert (dw - want).abs().max() <= 1e-12 * L1w.max()
        assert (L1w - torch.nn.grad.conv3d_weight(x.abs(), w.shape, dy.abs(), padding=1)).abs().max() <= 1e-12 * L1w.max()
        assert torch.equal(db, dy.sum((0, 2, 3, 4))) and torch.equal(L1b, dy.abs().sum((0, 2, 3, 4)))
        val, bound = ref.stats(a, A0, row.ci, 1, 8)
        assert torch.equal(val[:, 0], a.sum((0, 2, 3, 4))) and torch.equal(val[:, 1], (a * a).sum((0, 2, 3, 4))) and bool((bound > 0).all())


# channels of the weight gradient the emulation forms (every element of dw has the same sequence of voxels), and output channels of
# a large forward / data gradient (every output channel receives its products in the same order)
SUB = 2


def _conv_sub(row):
    return SUB if row.n * row.sp[0] * row.sp[1] * row.sp[2] * row.ci * row.co > 3e6 else None


def emulable(row, dtype, p, pl):
    """small enough, and a summation order tests/mfma_emu.py restates: not the strided data gradient (mode 1), and no weight gradient
    whose position lists pass 200 000 entries per wave slot (the two bf16t rows of 512 workgroups)"""
    if pl is None or not mc.runs(row, dtype, p):
        return False
    if p == "wgrad":
        return pl["p"] * pl["chain"] <= 200000
    return pl["mode"] == 0


def _emulated(row, dtype, fault=None, passes=None):
    pl = run.plans(row, dtype)
    inp = run.make_inputs(row, dtype)
    bnd = run.bounds(row, dtype, inp, pl)
    got, kept = {}, {}
    for p in passes or row.passes:
        if not emulable(row, dtype, p, pl[p]):
            continue
        if p == "wgrad":
            got.update(emu.wgrad(row, dtype, inp, pl[p], fault=fault, sub=SUB))
            kept["dw"] = tuple(t[:SUB, :SUB] for t in bnd["dw"])
            if row.dbias:
                kept["db"] = tuple(t[:SUB] for t in bnd["db"])
        else:
            sub = _conv_sub(row)
            res = emu.conv(row, dtype, inp, pl[p], p, fault=fault, sub=sub)
            got.update(res)
            kept.update({k: tuple(t[:sub] if k == "stats" else t[:, :sub] for t in bnd[k]) for k in res})
    return run.report(kept, got)


@pytest.mark.parametrize("row,dtype", mc.PAIRS, ids=mc.IDS)
def test_fp32_emulation_in_the_kernels_order_stays_inside_the_bounds(row, dtype):
    rep = _emulated(row, dtype)
    for name, ratio, over in rep:
        print("%s %s %-5s emulation: worst error / bound = %.3g" % (row.id, dtype, name, ratio))
        assert over == 0 and ratio <= 1, (row.id, dtype, name, ratio, over)


def test_the_emulation_reaches_every_kernel_and_storage_type():
    seen = set()
    for row, dtype in mc.PAIRS:
        for p, pl in run.plans(row, dtype).items():
            if emulable(row, dtype, p, pl):
                seen.add((pl["kernel"], dtype, p, pl["split"] if pl["kernel"] == "direct" else 0, bool(row.stats and p == "fwd")))
    for d in mc.DTYPES:
        for p in ("fwd", "dgrad"):
            assert ("tiled", d, p, 0, False) in seen and ("tiled_n8", d, p, 0, False) in seen, (d, p)
        assert ("tiled", d, "fwd", 0, True) in seen and ("direct", d, "fwd", 1, False) in seen and ("direct", d, "fwd", 0, False) in seen, d
        for k in ("cin1", "wgrad3") + (("wgrad6",) if d == "f32" else ("wgrad4", "bf16", "bf16t")):
            assert (k, d, "wgrad", 0, False) in seen, (k, d)
    assert ("direct", "f32", "dgrad", 1, False) in seen


# fault -> [(row, type, pass, the result that must leave its bound)]
MUST_FAIL = {
    "product-dropped-at-the-last-voxel": [("tile-ragged-5x9x17", "f32", "fwd", "y"), ("tile-ragged-5x9x17", "bf16", "fwd", "y"),
                                          ("stats-ragged-5x9x17", "f32", "fwd", "y"), ("kc24", "bf16", "dgrad", "dx"), ("kc24", "f32", "dgrad", "dx")],
    "single-group-channels-swapped": [("stats-ragged-5x9x17", "f32", "fwd", "y"), ("stats-kc48", "f32", "fwd", "y")],      # (the fp32 image only)
    # at weight 1e-3 only a small volume shows it in the values (the counted bound grows with sum |w| |x|); the device run
    # fills the neighbouring channels with NaN instead, which shows a stray read at any weight
    "neighbouring-channel-read": [("kc8-x-pitched-1x1x1", "f32", "fwd", "y"), ("kc8-x-pitched-1x1x1", "bf16", "fwd", "y")],
    "bf16-weights-unrounded": [("tile-ragged-5x9x17", "bf16", "fwd", "y"), ("kc24", "bf16", "dgrad", "dx"), ("nc8", "bf16", "fwd", "y")],
    "voxel-dropped-from-dw": [("tile-ragged-5x9x17", "f32", "wgrad", "dw"), ("tile-ragged-5x9x17", "bf16", "wgrad", "dw"),
                              ("wg3-ci8-co12", "f32", "wgrad", "dw"), ("wg3-ci8-co12", "bf16", "wgrad", "dw"), ("wg4-co12", "bf16", "wgrad", "dw"),
                              ("wg-cin1", "f32", "wgrad", "dw"), ("n64-512-units", "f32", "wgrad", "dw")],
    "w-halo-counted-into-dw": [("wg3-ci8-co12", "f32", "wgrad", "dw"), ("wg3-ci8-co12", "bf16", "wgrad", "dw"), ("wg4-co12", "bf16", "wgrad", "dw"),
                               ("wg-cin1", "bf16", "wgrad", "dw"), ("tile-ragged-5x9x17", "f32", "wgrad", "dw"),
                               ("tile-ragged-5x9x17", "bf16", "wgrad", "dw")],
    "db-doubled": [("nc8", "f32", "wgrad", "db"), ("ci8-co8", "f32", "wgrad", "db")],                                      # (the co8 forms are fp32)
    "statistics-include-the-bias": [("stats-ragged-5x9x17", "f32", "fwd", "stats"), ("stats-ragged-5x9x17", "bf16", "fwd", "stats")],
    "partial-dropped": [("stats-n3", "f32", "fwd", "stats"), ("stats-n3", "bf16", "fwd", "stats"), ("tile-ragged-5x9x17", "f32", "wgrad", "dw"),
                        ("tile-ragged-5x9x17", "bf16", "wgrad", "dw")],
    "last-ragged-row-unwritten": [("tile-ragged-5x9x17", "f32", "fwd", "y"), ("tile-ragged-5x9x17", "bf16", "fwd", "y"),
                                  ("stats-ragged-5x9x17", "f32", "fwd", "y")],
}


def test_every_deliberate_error_is_listed():
    assert set(MUST_FAIL) == set(emu.FAULTS) and len(emu.FAULTS) == 10


@pytest.mark.parametrize("fault", emu.FAULTS)
def test_deliberate_error_leaves_the_bounds(fault):
    for rid, dtype, p, name in MUST_FAIL[fault]:
        rep = {k: (ratio, over) for k, ratio, over in _emulated(ROWS[rid], dtype, fault=fault, passes=(p,))}
        ratio, over = rep[name]
        print("%s on %s %s %s: %s worst error / bound = %.3g, %d elements over" % (fault, rid, dtype, p, name, ratio, over))
        assert over > 0 and ratio > 1, (fault, rid, dtype, p, name, ratio)
        if name == "stats":          # a statistics fault leaves y alone
            assert rep["y"][1] == 0
