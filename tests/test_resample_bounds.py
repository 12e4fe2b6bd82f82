"""CPU suite: the bounds of tests/test_resample_parity_gpu.py are neither too tight for correct fp32 arithmetic nor too loose to see
an error.

  acceptance  torch's own fp32 results on the CPU (F.max_pool3d, F.interpolate and their autograd) stay inside the bounds for every
              parity row of at most 2^22 output elements (trilinear rows: the slab kernels' bound, whose coordinate term covers
              ATen's expression), and so does an fp32 emulation of the expression order of the three x2 kernels under their own;
  detection   the comparison flags five deliberate errors applied to a copy of the reference result."""
import pytest
import torch

import resample_cases as rc
import resample_ref as rr
import resample_run as run
import test_resample_parity_gpu as parity

SMALL = [(r, t) for r, t in rc.PARITY_PAIRS if rc.N * r.c * max(torch.Size(run.out_size(r)).numel(), torch.Size(r.sp).numel()) <= 1 << 22]
SMALL_IDS = [i for i, (r, t) in zip(rc.PARITY_IDS, rc.PARITY_PAIRS) if (r, t) in SMALL]
SLAB = {"fwd": "upsample_fwd", "bwd": "tables+upsample_bwd"}


def _assert_inside(row, dtype, ref, names, got, who):
    rep = parity.report(row, dtype, ref, names, got)
    bad = ["%s: %d elements over, worst error / bound %.3f" % r for r in rep if r[2]]
    assert not bad, "%s %s, %s:\n  %s" % (row.id, dtype, who, "\n  ".join(bad))
    return rep


@pytest.mark.parametrize("row,dtype", SMALL, ids=SMALL_IDS)
def test_bounds_accept_torch_cpu_fp32(row, dtype):
    inp = run.make_inputs(row, dtype)
    ref = run.reference(row, inp)
    cpu = run.cpu_fp32(row, inp)
    got = {k: v.to(run.TORCH[dtype]) for k, v in cpu.items()}
    _assert_inside(row, dtype, ref, SLAB, got, "torch CPU fp32")


# ---------------------------------------------------------------------------------------------- fp32 emulation of the x2 kernels
def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64"""
    a = torch.as_tensor(a, dtype=torch.float64) if not torch.is_tensor(a) else a.double()
    return (a * b.double() + c.double()).float()


def _nb(x, dim):
    """(self, neighbour) along `dim` at fine positions: coarse o >> 1 and the one before (o even) or after (o odd), clamped"""
    s = x.shape[dim]
    o = torch.arange(2 * s)
    i0 = o >> 1
    i1 = (i0 + torch.where(o % 2 == 1, 1, -1)).clamp(0, s - 1)
    return x.index_select(dim, i0), i1


def emulate_fwd_march(x):
    """upsample2x_fwd_march_kernel: in-plane P at fine (h, w), then the two fine planes of every coarse plane"""
    xh, h1 = _nb(x, 3)
    xh1 = x.index_select(3, h1)
    a, w1 = _nb(xh, 4)
    b, c, d = xh.index_select(4, w1), _nb(xh1, 4)[0], xh1.index_select(4, w1)
    p = (0.75 * _fma(0.75, a, 0.25 * b)).float() + 0.25 * _fma(0.75, c, 0.25 * d)      # not contracted: one rounding more
    pd, d1 = _nb(p, 2)
    return _fma(0.75, pd, 0.25 * p.index_select(2, d1))


def _w2(i, s):
    w = torch.tensor([0.25, 0.75, 0.75, 0.25]).repeat(s, 1)
    w[0, 0], w[0, 1] = 0.0, 1.0
    w[s - 1, 2], w[s - 1, 3] = 1.0, 0.0
    if s == 1:
        w[0] = torch.tensor([0.0, 1.0, 1.0, 0.0])
    return w            # (s, 4): up2_axis_weights


def _taps(dy, dim, s):
    """the four fine slices 2i-1 .. 2i+2 along dim for every coarse i, zeros outside"""
    pad = [0, 0] * (4 - dim) + [1, 1]
    p = torch.nn.functional.pad(dy, pad)
    return [p.index_select(dim, torch.arange(s) * 2 + a) for a in range(4)]


def _wv(w, a, dim):
    shape = [1] * 5
    shape[dim] = -1
    return w[:, a].reshape(shape)


def emulate_bwd_tile(dy, sp):
    """upsample2x_bwd_kernel: 64 fmas in (a, b, c) order with the exact weight products"""
    wd, wh, ww = (_w2(None, s) for s in sp)
    acc = torch.zeros(dy.shape[:2] + tuple(sp))
    for a, ta in enumerate(_taps(dy, 2, sp[0])):
        for b, tb in enumerate(_taps(ta, 3, sp[1])):
            wab = _wv(wd, a, 2) * _wv(wh, b, 3)
            for c, tc in enumerate(_taps(tb, 4, sp[2])):
                acc = _fma(wab * _wv(ww, c, 4), tc, acc)
    return acc


def emulate_bwd_march(dy, sp):
    """upsample2x_bwd_march_kernel: per fine plane the row sums r, then S_f over the rows, then the D taps as a running sum"""
    wd, wh, ww = (_w2(None, s) for s in sp)
    sf = torch.zeros(dy.shape[:3] + tuple(sp[1:]))
    for b, tb in enumerate(_taps(dy, 3, sp[1])):
        r = torch.zeros_like(sf)
        for c, tc in enumerate(_taps(tb, 4, sp[2])):
            r = _fma(_wv(ww, c, 4), tc, r)
        sf = _fma(_wv(wh, b, 3), r, sf)
    t = _taps(sf, 2, sp[0])
    acc = (_wv(wd, 0, 2) * t[0]).float()
    for a in (1, 2, 3):
        acc = _fma(_wv(wd, a, 2), t[a], acc)
    return acc


X2 = [(r, t) for r, t in SMALL if not run.is_pool(r) and r.fwd[t].startswith("upsample2x_fwd_march")]


@pytest.mark.parametrize("row,dtype", X2, ids=["%s-%s" % (r.id, t) for r, t in X2])
def test_bounds_accept_an_fp32_emulation_of_the_x2_kernels(row, dtype):
    inp = run.make_inputs(row, dtype)
    ref = run.reference(row, inp)
    st = run.TORCH[dtype]
    y = emulate_fwd_march(inp["x"].float()).to(st)
    for bwd, emu in (("upsample2x_bwd_march", emulate_bwd_march), ("upsample2x_bwd", emulate_bwd_tile)):
        got = {"y": y, "dx": emu(inp["dy"].float(), row.sp).to(st)}
        _assert_inside(row, dtype, ref, {"fwd": "upsample2x_fwd_march", "bwd": bwd}, got, "emulation with " + bwd)


# ---------------------------------------------------------------------------------------------- detection
def _row(rows, rid):
    return next(r for r in rows if r.id == rid)


def _case(row, dtype="f32"):
    inp = run.make_inputs(row, dtype)
    ref = run.reference(row, inp)
    names = {"fwd": row.fwd[dtype], "bwd": row.bwd[dtype]}
    got = {"y": ref["y"].to(run.TORCH[dtype]), "dx": ref["dx"].to(run.TORCH[dtype])}
    return inp, ref, names, got


def _over(row, dtype, ref, names, got):
    return {k: over for k, _, over in parity.report(row, dtype, ref, names, got)}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_reference_itself_passes(dtype):
    for row in (_row(rc.PARITY_UP, "x2_c20_two_passes"), _row(rc.PARITY_POOL, "ties_k2"), _row(rc.PARITY_UP, "old_nearest_size")
                if dtype == "f32" else _row(rc.PARITY_UP, "nearest_x1_5")):
        inp, ref, names, got = _case(row, dtype)
        assert _over(row, dtype, ref, names, got) == {"y": 0, "dx": 0}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_detects_swapped_weights_on_one_fine_plane_at_a_segment_seam(dtype):
    row = _row(rc.PARITY_UP, "x2_c20_two_passes")          # segments of 4 coarse planes: fine plane 8 opens the second one
    inp, ref, names, got = _case(row, dtype)
    got["y"][:, :, 8] = got["y"][:, :, 7]                   # 0.25 P_4 + 0.75 P_3 is what fine plane 7 holds
    over = _over(row, dtype, ref, names, got)
    assert over["y"] > 0 and over["dx"] == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_detects_one_tap_dropped_at_a_tile_border(dtype):
    row = _row(rc.PARITY_UP, "old_march_c24" if dtype == "f32" else "old_bf16_c40")    # tile kernel: 2 x 4 x 16 coarse tiles
    inp, ref, names, got = _case(row, dtype)
    i = (0, 3, 1, 3, 15)                                    # last row and column of the first tile: the taps 2i+2 come from the halo
    dy = inp["dy"].double()
    lost = 0.75 * 0.25 * 0.25 * dy[0, 3, 2 * 1, 2 * 3 + 2, 2 * 15 + 2]
    assert lost != 0
    got["dx"][i] = (ref["dx"][i] - lost).to(got["dx"].dtype)
    over = _over(row, dtype, ref, names, got)
    assert over["dx"] == 1 and over["y"] == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_detects_the_last_maximum_taken_on_a_tie(dtype):
    row = _row(rc.PARITY_POOL, "ties_k2")
    inp, ref, names, got = _case(row, dtype)
    x, dy = inp["x"].double(), inp["dy"].double()
    # the last maximum in raster order is the first one of the mirrored tensor (kernel 2, stride 2, even extents)
    _, tap_m = rr.pool_fwd(x.flip(2, 3, 4), row.k, row.s, row.p)
    tap_last = 7 - tap_m.flip(2, 3, 4)
    assert bool((tap_last != ref["tap"]).any())
    got["dx"] = rr.pool_bwd(dy, tap_last, x.shape, row.k, row.s, row.p)[0].to(got["dx"].dtype)
    over = _over(row, dtype, ref, names, got)
    assert over["dx"] > 0 and over["y"] == 0                # the values are the same: only the gradient shows the index


@pytest.mark.parametrize("rid", ["old_nearest_size", "old_trilinear_size", "nearest_x1_5", "trilinear_down"])
def test_detects_a_source_index_off_by_one_in_w(rid):
    row = _row(rc.PARITY_UP, rid)
    inp, ref, names, got = _case(row)
    x, out = inp["x"].double(), run.out_size(row)
    ow = out[2] // 2
    if row.mode == "nearest":
        shifted = x[..., 1:]
        wrong = rr.nearest_fwd(torch.cat([shifted, shifted[..., -1:]], -1), out, run.ratios(row))
    else:
        shifted = torch.cat([x[..., 1:], x[..., -1:]], -1)
        wrong = rr.trilinear_fwd(shifted, out, run.ratios(row), bool(row.ac))[0]
    got["y"][..., ow] = wrong[..., ow].to(got["y"].dtype)
    over = _over(row, "f32", ref, names, got)
    assert over["y"] > 0.9 * wrong[..., ow].numel() and over["dx"] == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_detects_a_channel_quad_of_the_second_pass_left_unwritten(dtype):
    row = _row(rc.PARITY_UP, "x2_c20_two_passes")          # passes of 16 channels: the quad 16..19 is the second pass's only one
    inp, ref, names, got = _case(row, dtype)
    for stale in (0.0, float("nan")):
        bad = {k: v.clone() for k, v in got.items()}
        bad["y"][1, 16:20, 9, 5, 11] = stale
        over = _over(row, dtype, ref, names, bad)
        assert over["y"] == 4 and over["dx"] == 0
