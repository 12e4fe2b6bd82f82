"""What the parity rows of tests/resample_cases.py (ParityPool, ParityUp) mean: their geometries and the launch plans the library
answers for them (host only), their inputs, their float64 reference (tests/resample_ref.py), and how they run through the public
API on the device."""
import math

import torch

import resample_cases as rc
import resample_ref as rr
from mri_epilepsy_diagnosis_amd import ops
from mri_epilepsy_diagnosis_amd._lib import BF16, F32, PASS_DGRAD, PASS_FWD, UP_NEAREST, UP_TRILINEAR, PoolGeom, UpGeom

TYPES = {"f32": F32, "bf16": BF16}
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}
ESZ = {"f32": 4, "bf16": 2}
CL3D = torch.channels_last_3d


def is_pool(row):
    return isinstance(row, rc.ParityPool)


def slice_align(layout, dtype):
    """ptr_align of the channel slice `layout` = (width, off) of a buffer (whose base the allocator and the guard keep at 256 bytes)"""
    off = layout[1] * ESZ[dtype] if layout else 0
    return min(16, off & -off) if off else 16


def _ld(row, name):
    return row.layout[name][0] if name in row.layout else row.c


def out_size(row):
    if is_pool(row):
        return tuple(rr.pool_out(i, k, s, p) for i, k, s, p in zip(row.sp, row.k, row.s, row.p))
    if row.size is not None:
        return tuple(row.size)
    return tuple(int(math.floor(float(i) * float(row.scale))) for i in row.sp)


def ratios(row):
    """the source step per destination step ops.upsample3d hands to the library (torch's)"""
    out = out_size(row)
    if row.mode == "trilinear" and row.ac:
        return [(i - 1) / (o - 1) if o > 1 else 0.0 for i, o in zip(row.sp, out)]
    return [1.0 / float(row.scale) if row.scale is not None else i / o for i, o in zip(row.sp, out)]


def plans(row, dtype, aligns=None):
    """{"fwd" | "bwd": (kernel name, plan numbers)} of the row: ops.pool_route / pool_plan or ops.upsample_route / upsample_plan.
    aligns: {"fwd" | "bwd": ptr_align of the pass's tensors}; by default what the row's layout gives fresh allocations and slices."""
    al = {"fwd": min(slice_align(row.layout.get(k), dtype) for k in ("x", "out")),
          "bwd": min(slice_align(row.layout.get(k), dtype) for k in ("dy", "dskip"))}
    al.update(aligns or {})
    n, out = rc.N, out_size(row)
    if is_pool(row):
        gf = PoolGeom(n, *row.sp, *out, row.c, *row.k, *row.s, *row.p, _ld(row, "x"), row.c, TYPES[dtype])
        gb = PoolGeom(n, *row.sp, *out, row.c, *row.k, *row.s, *row.p, row.c, _ld(row, "dy"), TYPES[dtype])
        add = _ld(row, "dskip") if row.addend else 0
        return {"fwd": (ops.pool_route(gf, PASS_FWD, align=al["fwd"]), ops.pool_plan(gf, PASS_FWD, align=al["fwd"])),
                "bwd": (ops.pool_route(gb, PASS_DGRAD, addend_ld=add, align=al["bwd"]), ops.pool_plan(gb, PASS_DGRAD, addend_ld=add, align=al["bwd"]))}
    mode = UP_NEAREST if row.mode == "nearest" else UP_TRILINEAR
    gf = UpGeom(n, *row.sp, *out, row.c, _ld(row, "x"), _ld(row, "out"), mode, 1 if row.ac else 0, *ratios(row), TYPES[dtype])
    gb = UpGeom(n, *row.sp, *out, row.c, row.c, _ld(row, "dy"), mode, 1 if row.ac else 0, *ratios(row), TYPES[dtype])
    return {"fwd": (ops.upsample_route(gf, PASS_FWD, align=al["fwd"]), ops.upsample_plan(gf, PASS_FWD, align=al["fwd"])),
            "bwd": (ops.upsample_route(gb, PASS_DGRAD, align=al["bwd"]), ops.upsample_plan(gb, PASS_DGRAD, align=al["bwd"]))}


def declared_mismatches(row, dtype, got):
    """what of the row's declared names and numbers `got` (= plans(...)) does not give"""
    wrong = []
    for pass_, want in (("fwd", row.fwd[dtype]), ("bwd", row.bwd[dtype])):
        if got[pass_][0] != want:
            wrong.append("%s %s %s: declares %s, runs %s" % (row.id, dtype, pass_, want, got[pass_][0]))
        for field, v in row.nums.get(pass_, {}).items():
            v = v[dtype] if isinstance(v, dict) else v
            if got[pass_][1][field] != v:
                wrong.append("%s %s %s: declares %s = %d, the plan has %d" % (row.id, dtype, pass_, field, v, got[pass_][1][field]))
    return wrong


# ---------------------------------------------------------------------------------------------- inputs and reference
def _stored(t, dtype):
    return t.to(TORCH[dtype])


def make_inputs(row, dtype, seed=0):
    """{x, dy, addend}: logical (N, C, D, H, W) CPU tensors of the storage type"""
    g = torch.Generator().manual_seed(seed + 17 * len(row.id))
    shape = (rc.N, row.c) + tuple(row.sp)
    x = torch.randn(shape, generator=g)
    values = row.values if is_pool(row) else "normal"
    if values == "ties":
        x = torch.randint(0, 8, shape, generator=g).float() * 0.375 - 1.5
    elif values == "negative":
        x = -x.abs() - 1.0
    elif values == "nan":
        x[torch.rand(shape, generator=g) < 0.04] = float("nan")
    elif values == "neginf":
        x[:, :, :, : max(2, row.sp[1] // 2)] = -float("inf")
        x[:, : max(1, row.c // 2), : max(2, row.sp[0] // 2)] = -float("inf")
    inp = {"x": _stored(x, dtype), "dy": _stored(torch.randn((rc.N, row.c) + out_size(row), generator=g), dtype)}
    if is_pool(row) and row.addend:
        inp["addend"] = _stored(torch.randn(shape, generator=g), dtype)
    return inp


def reference(row, inp, sensitivity=(True, True)):
    """float64 results and the magnitudes of their bounds (see tests/test_resample_parity_gpu.py), from the stored inputs.
    sensitivity: whether the (forward, backward) bound has a coordinate term — the x2 kernels' has none, their weights are exact."""
    x, dy = inp["x"].double(), inp["dy"].double()
    ref = {}
    if is_pool(row):
        ref["y"], ref["tap"] = rr.pool_fwd(x, row.k, row.s, row.p)
        ref["dx"], ref["dx_l1"], ref["dx_t"] = rr.pool_bwd(dy, ref["tap"], x.shape, row.k, row.s, row.p,
                                                            inp["addend"].double() if row.addend else None)
    elif row.mode == "nearest":
        ref["y"] = rr.nearest_fwd(x, out_size(row), ratios(row))
        ref["dx"], ref["dx_l1"], ref["dx_t"] = rr.nearest_bwd(dy, row.sp, ratios(row))
    else:
        ref["y"], ref["y_a"], ref["y_g"] = rr.trilinear_fwd(x, out_size(row), ratios(row), bool(row.ac), sensitivity[0])
        ref["dx"], ref["dx_l1"], ref["dx_t"], ref["dx_g"] = rr.trilinear_bwd(dy, row.sp, ratios(row), bool(row.ac), sensitivity[1])
    return ref


def cpu_fp32(row, inp):
    """{y, dx}: torch on the CPU in fp32 (F.max_pool3d / F.interpolate and their autograd) on the stored inputs"""
    import torch.nn.functional as F
    x = inp["x"].float().requires_grad_(True)
    if is_pool(row):
        y = F.max_pool3d(x, row.k, row.s, row.p)
    else:
        kw = dict(size=row.size) if row.size is not None else dict(scale_factor=row.scale)
        y = F.interpolate(x, mode=row.mode, align_corners=row.ac if row.mode == "trilinear" else None, **kw)
    grads = [inp["dy"].float()]
    outs = [y]
    if is_pool(row) and row.addend:
        outs.append(x * 1.0)
        grads.append(inp["addend"].float())
    torch.autograd.backward(outs, grads)
    return {"y": y.detach(), "dx": x.grad}


# ---------------------------------------------------------------------------------------------- the device run
def _place(t, layout, device):
    """t on the device: dense NDHWC, or the channel slice `layout` of a sentinel-filled wider buffer -> (tensor, SentinelSlice | None)"""
    import guard
    if layout is None:
        return t.to(device).contiguous(memory_format=CL3D), None
    ss = guard.SentinelSlice(t.shape[0], layout[0], tuple(t.shape[2:]), t.dtype, layout[1], t.shape[1], device=device)
    ss.slice.copy_(t.to(device))
    return ss.slice, ss


def run_row(row, dtype, inp, device="cuda", check_plan=True):
    """({y, dx} on the device, [(what, SentinelSlice)], problems of the declared plan with the tensors' real alignments).  Inputs that
    are slices sit among NaN sentinels: a read outside the slice that reaches a result shows as NaN there."""
    import guard
    guards = []

    def place(name, key):
        t, ss = _place(inp[name], row.layout.get(key), device)
        if ss is not None:
            guards.append((key, ss))
        return t
    x = place("x", "x").detach().requires_grad_(True)
    dy = place("dy", "dy")
    dskip = place("addend", "dskip") if is_pool(row) and row.addend else None
    out = None
    if "out" in row.layout and not is_pool(row):
        width, off = row.layout["out"]
        out = guard.SentinelSlice(rc.N, width, out_size(row), TORCH[dtype], off, row.c, device=device)
        guards.append(("out", out))
    wrong = []
    if check_plan:
        aligns = {"fwd": ops._ptr_align(x, out.slice if out is not None else None), "bwd": ops._ptr_align(dy, dskip)}
        wrong = declared_mismatches(row, dtype, plans(row, dtype, aligns))
        assert not wrong, "\n".join(wrong)
    if is_pool(row):
        if row.addend:
            y, skip = ops.max_pool3d_skip(x, row.k, row.s, row.p)
            torch.autograd.backward([y, skip], [dy, dskip])
        else:
            y = ops.max_pool3d(x, row.k, row.s, row.p)
            y.backward(dy)
    else:
        y = ops.upsample3d(x, size=row.size, scale_factor=row.scale, mode=row.mode, align_corners=row.ac if row.mode == "trilinear" else None,
                           out=(out.buf, row.layout["out"][1]) if out is not None else None)
        y.backward(dy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": x.grad.detach()}, guards
