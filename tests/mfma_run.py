"""What the rows of tests/mfma_cases.py mean: their geometries, the route names and launch plans the library answers for them (host
only), their inputs, their float64 reference with the counted bounds (tests/mfma_ref.py), and how they run through the raw entry
points mri3d_conv3d_fwd / _fwd_stats / _dgrad / _wgrad and the *_cat forms on guarded device buffers (tests/guard.py)."""
import ctypes

import torch

import mfma_cases as mc
import mfma_ref as ref
from mri_epilepsy_diagnosis_amd import _lib, ops
from mri_epilepsy_diagnosis_amd._lib import BF16, F32, PASS_DGRAD, PASS_FWD, PASS_WGRAD, ConvGeom

TYPES = {"f32": F32, "bf16": BF16}
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}
ESZ = {"f32": 4, "bf16": 2}
PASSES = {"fwd": PASS_FWD, "dgrad": PASS_DGRAD, "wgrad": PASS_WGRAD}
EINVAL, ENOTSUP, EWORKSPACE = -1, -2, -4
NAN = float("nan")


def width(row, name):
    dense = {"x": row.split or row.ci, "x2": row.ci - row.split, "y": row.co}[name]
    return row.layout[name][0] if name in row.layout else dense


def off(row, name):
    return row.layout[name][1] if name in row.layout else 0


def out_sp(row):
    return tuple((e - 1) // row.stride + 1 for e in row.sp)          # k = 3, padding 1


def align(row, dtype, side):
    """largest power of two <= 16 dividing the byte offset of the side's slices from their 256-byte aligned buffers: "x" = x (dx)
    and with a split x2 (dx2), "y" = y (dy)"""
    bits = 16
    for name in (("x", "x2") if row.split else ("x",)) if side == "x" else ("y",):
        bits |= off(row, name) * ESZ[dtype]
    return bits & -bits


# ---------------------------------------------------------------------------------------------- geometries, routes and plans
def geom(row, dtype):
    """the ConvGeom the entry points get: x_ld = the pitch of x (of the first tensor of a split operand), y_ld that of y"""
    D, H, W = row.sp
    Do, Ho, Wo = out_sp(row)
    s = row.stride
    return ConvGeom(row.n, D, H, W, row.ci, Do, Ho, Wo, row.co, 3, 3, 3, s, s, s, 1, 1, 1, 1, 1, 1, width(row, "x"), width(row, "y"),
                    TYPES[dtype])


def call(row, p):
    """the arguments of mri3d_conv3d_route / _mfma_plan_query that describe the row's call of the pass, after (g, pass)"""
    stats = row.stats and p == "fwd"
    bias = (row.bias and p == "fwd") or (row.dbias and p == "wgrad")
    return dict(stats=stats, bias=bias, split=row.split, second_ld=width(row, "x2") if row.split else 0)


def route(row, dtype, p, x_align=None, y_align=None):
    xa = align(row, dtype, "x") if x_align is None else x_align
    ya = align(row, dtype, "y") if y_align is None else y_align
    return ops.conv_route(geom(row, dtype), PASSES[p], x_align=xa, y_align=ya, **call(row, p))


def plan(row, dtype, p, x_align=None, y_align=None):
    """plan numbers of the pass (ops.conv_mfma_plan) with the route name under "route", or None where the query refuses"""
    xa = align(row, dtype, "x") if x_align is None else x_align
    ya = align(row, dtype, "y") if y_align is None else y_align
    try:
        pl = ops.conv_mfma_plan(geom(row, dtype), PASSES[p], x_align=xa, y_align=ya, **call(row, p))
    except _lib.Mri3dError:
        return None
    pl["route"] = route(row, dtype, p, xa, ya)
    return pl


def plans(row, dtype, aligns=None):
    """aligns: {"x" | "y": alignment of the real pointers} instead of what the layout gives"""
    a = aligns or {}
    return {p: plan(row, dtype, p, a.get("x"), a.get("y")) for p in row.passes}


def declared_mismatches(row, dtype, got):
    """what of the row's declarations `got` (= plans(...)) does not give: plan numbers, route names, and the passes it says the
    query refuses (because the entry point refuses: `refused`, or because the call leaves the family: `leaves`)"""
    wrong = []
    for p in row.passes:
        if (got[p] is None) != (not mc.runs(row, dtype, p)):
            wrong.append("%s %s %s: declared %s, the query %s" % (row.id, dtype, p, "served" if mc.runs(row, dtype, p) else "not served",
                                                                 "refuses" if got[p] is None else "serves"))
    for p, d in mc.declared(row, dtype).items():
        for f, v in d.items():
            if got.get(p) is not None and got[p][f] != v:
                wrong.append("%s %s %s: declares %s = %r, the plan has %r" % (row.id, dtype, p, f, v, got[p][f]))
    for p in row.passes:
        name = route(row, dtype, p)
        if p in row.refused.get(dtype, ()) and name != "none":
            wrong.append("%s %s %s: declared refused, the route is %r" % (row.id, dtype, p, name))
        if p in row.leaves.get(dtype, ()) and name.split()[0] not in ("generic", "pointwise", "march"):
            wrong.append("%s %s %s: declared to leave the family, the route is %r" % (row.id, dtype, p, name))
    return wrong


# ---------------------------------------------------------------------------------------------- inputs, reference, bounds
def _uniform(shape, g):
    return torch.rand(shape, generator=g) + 0.5          # [0.5, 1.5): a dropped part of a sum cannot cancel


def make_inputs(row, dtype, seed=0):
    """logical NCDHW CPU tensors: activations of the storage type, weights and bias fp32"""
    g = torch.Generator().manual_seed(seed + 31 * len(row.id) + sum(map(ord, row.id)))
    st = TORCH[dtype]
    return {"x": _uniform((row.n, row.ci) + row.sp, g).to(st), "dy": _uniform((row.n, row.co) + out_sp(row), g).to(st),
            "w": torch.randn((row.co, row.ci, 3, 3, 3), generator=g), "b": torch.randn(row.co, generator=g) if row.bias else None}


def bounds(row, dtype, inp, pl):
    """{name: (float64 reference, elementwise bound)} of the passes that run; pl = plans(row, dtype)"""
    out = {}
    x, dy = inp["x"].double(), inp["dy"].double()
    if mc.runs(row, dtype, "fwd"):
        q = pl["fwd"]
        w = ref.stored_weights(inp["w"], dtype, q["kernel"])
        y, A, a, A0 = ref.forward(x, w, inp["b"].double() if inp["b"] is not None else None, row.stride)
        out["y"] = (y, ref.stored_bound(y, A, row.ci, dtype, 3 if q["kernel"] == "direct" and q["split"] else 0))
        if row.stats:
            out["stats"] = ref.stats(a, A0, row.ci, q["max_tasks"], q["grid"])
    if mc.runs(row, dtype, "dgrad"):
        q = pl["dgrad"]
        w = ref.stored_weights(inp["w"], dtype, q["kernel"])
        dx, L1 = ref.dgrad(dy, w, (row.n, row.ci) + row.sp, row.stride)
        out["dx"] = (dx, ref.stored_bound(dx, L1, row.co, dtype, 3 if q["kernel"] == "direct" and q["split"] else 0))
    if mc.runs(row, dtype, "wgrad"):
        q = pl["wgrad"]
        dw, L1w, db, L1b = ref.wgrad(x, dy, row.co)
        out["dw"] = (dw, ref.wgrad_bound(L1w, q["chain"], q["p"]))
        if row.dbias:
            out["db"] = (db, ref.wgrad_bound(L1b, q["chain"], q["p"]))
    return out


def report(bnd, got):
    """[(name, worst error / bound, elements over)]: every element of every result"""
    assert set(bnd) == set(got), (sorted(bnd), sorted(got))
    return [(k,) + ref.compare(want, b, got[k]) for k, (want, b) in bnd.items()]


# ---------------------------------------------------------------------------------------------- the device run
def _input(t, w, o, device):
    """logical NCDHW `t` as the channel slice [o, o + c) of an NDHWC buffer of `w` channels whose other channels hold NaN"""
    n, c = t.shape[:2]
    buf = torch.full((n,) + tuple(t.shape[2:]) + (w,), NAN, dtype=t.dtype, device=device)
    view = buf.permute(0, 4, 1, 2, 3).narrow(1, o, c)
    view.copy_(t.to(device))
    return view


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr_align(*ts):
    bits = 16
    for t in ts:
        if t is not None:
            bits |= t.data_ptr()
    return bits & -bits


def pointer_aligns(row, dtype, device="cuda"):
    """{"x" | "y": alignment} of the slices as the device buffers of `run` place them (every buffer starts 256-byte aligned)"""
    def one(name, c):
        return _input(torch.zeros((1, c, 1, 1, 1), dtype=TORCH[dtype]), width(row, name), off(row, name), device)
    c1 = row.split or row.ci
    return {"x": _ptr_align(one("x", c1), one("x2", row.ci - c1) if row.split else None), "y": _ptr_align(one("y", row.co))}


class Outputs:
    """the guarded buffers of one run, the return codes, the results on the host, and the alignment of the pointers handed over"""

    def __init__(self):
        self.slices, self.flat, self.got, self.rcs, self.untouched, self.aligns, self.tails = [], [], {}, {}, {}, {}, {}

    def check(self, what):
        for name, ss in self.slices:
            ss.assert_outside_intact("%s: %s" % (what, name))
        for name, g in self.flat:
            g.assert_guards_intact("%s: %s" % (what, name))
        for name, ok in self.tails.items():
            assert ok, "%s: %s written past the bytes the plan asks for" % (what, name)


def run(row, dtype, inp, pl, device="cuda", passes=None, short_ws=False):
    """The row's passes through the raw entry points -> Outputs.  pl = plans(row, dtype): the workspace is stated with the plan's
    size (short_ws: one byte less) and the bytes behind it must stay untouched.  passes: instead of those the plan serves (a pass
    the query refuses gets the size mri3d_conv3d_workspace_bytes names)."""
    import guard
    L = _lib.lib()
    g = geom(row, dtype)
    st = TORCH[dtype]
    c1 = row.split or row.ci
    x2w = width(row, "x2") if row.split else 0
    o = Outputs()
    w = inp["w"].to(device).contiguous()

    def workspace(p):
        general = int(L.mri3d_conv3d_workspace_bytes(ctypes.byref(g), PASSES[p]))
        need = pl[p]["workspace_bytes"] if pl.get(p) else general
        ws = guard.guarded(max(general, need, 256) // 4 + 64, torch.float32, device=device)
        o.flat.append(("workspace " + p, ws))
        return ws, need - (1 if short_ws else 0), need

    def tail(p, ws, need):
        o.tails["workspace " + p] = bool(ws.untouched()[(need + 3) // 4:].all())
        o.untouched["workspace " + p] = bool(ws.untouched().all())

    todo = passes if passes is not None else [p for p in row.passes if mc.runs(row, dtype, p)]
    if "fwd" in todo or "wgrad" in todo:
        x = _input(inp["x"][:, :c1], width(row, "x"), off(row, "x"), device)
        x2 = _input(inp["x"][:, c1:], x2w, off(row, "x2"), device) if row.split else None
    if "dgrad" in todo or "wgrad" in todo:
        dy = _input(inp["dy"], width(row, "y"), off(row, "y"), device)
    if "fwd" in todo:
        b = inp["b"].to(device).contiguous() if inp["b"] is not None else None
        y = guard.SentinelSlice(row.n, width(row, "y"), out_sp(row), st, off(row, "y"), row.co, device=device)
        o.slices.append(("y", y))
        part = None
        if row.stats:
            nb = pl["fwd"]["stats_blocks"] if pl.get("fwd") else 16
            part = guard.guarded((max(nb, 1), row.co, 2), torch.float64, device=device)      # the sentinel is a NaN
            o.flat.append(("stat_partials", part))
        ws, wsb, need = workspace("fwd")
        o.aligns["fwd"] = {"x": _ptr_align(x, x2), "y": _ptr_align(y.slice)}
        if row.split:
            o.rcs["fwd"] = L.mri3d_conv3d_fwd_cat(ctypes.byref(g), _p(x), _p(x2), row.split, x2w, _p(w), _p(b), _p(y.slice),
                                                  _p(part.flat) if part is not None else None, _p(ws.flat), wsb, _stream())
        elif row.stats:
            o.rcs["fwd"] = L.mri3d_conv3d_fwd_stats(ctypes.byref(g), _p(x), _p(w), _p(b), _p(y.slice), _p(part.flat), _p(ws.flat), wsb, _stream())
        else:
            o.rcs["fwd"] = L.mri3d_conv3d_fwd(ctypes.byref(g), _p(x), _p(w), _p(b), _p(y.slice), _p(ws.flat), wsb, _stream())
        torch.cuda.synchronize()
        tail("fwd", ws, need)
        o.got["y"] = y.slice.detach().cpu().contiguous()
        o.untouched["y"] = bool(y.slice_untouched().all())
        if part is not None:
            o.got["stats"] = part.region.cpu().sum(0)
            o.untouched["stats"] = bool(part.untouched().all())
    if "dgrad" in todo:
        dx = guard.SentinelSlice(row.n, width(row, "x"), row.sp, st, off(row, "x"), c1, device=device)
        o.slices.append(("dx", dx))
        dx2 = guard.SentinelSlice(row.n, x2w, row.sp, st, off(row, "x2"), row.ci - c1, device=device) if row.split else None
        if dx2 is not None:
            o.slices.append(("dx2", dx2))
        ws, wsb, need = workspace("dgrad")
        o.aligns["dgrad"] = {"x": _ptr_align(dx.slice, dx2.slice if dx2 is not None else None), "y": _ptr_align(dy)}
        if row.split:
            o.rcs["dgrad"] = L.mri3d_conv3d_dgrad_cat(ctypes.byref(g), _p(dy), _p(w), _p(dx.slice), _p(dx2.slice), row.split, x2w, _p(ws.flat),
                                                      wsb, _stream())
        else:
            o.rcs["dgrad"] = L.mri3d_conv3d_dgrad(ctypes.byref(g), _p(dy), _p(w), None, _p(dx.slice), _p(ws.flat), wsb, _stream())
        torch.cuda.synchronize()
        tail("dgrad", ws, need)
        parts = [dx.slice.detach().cpu()] + ([dx2.slice.detach().cpu()] if dx2 is not None else [])
        o.got["dx"] = torch.cat(parts, 1).contiguous()
        o.untouched["dx"] = bool(dx.slice_untouched().all()) and (dx2 is None or bool(dx2.slice_untouched().all()))
    if "wgrad" in todo:
        dw = guard.guarded((row.co, row.ci, 3, 3, 3), torch.float32, device=device)
        db = guard.guarded((row.co,), torch.float32, device=device) if row.dbias else None
        o.flat += [("dw", dw)] + ([("db", db)] if db is not None else [])
        ws, wsb, need = workspace("wgrad")
        o.aligns["wgrad"] = {"x": _ptr_align(x, x2), "y": _ptr_align(dy)}
        if row.split:
            o.rcs["wgrad"] = L.mri3d_conv3d_wgrad_cat(ctypes.byref(g), _p(x), _p(x2), row.split, x2w, _p(dy), _p(dw.flat),
                                                      _p(db.flat) if db is not None else None, _p(ws.flat), wsb, _stream())
        else:
            o.rcs["wgrad"] = L.mri3d_conv3d_wgrad(ctypes.byref(g), _p(x), _p(dy), _p(dw.flat), _p(db.flat) if db is not None else None,
                                                  _p(ws.flat), wsb, _stream())
        torch.cuda.synchronize()
        tail("wgrad", ws, need)
        o.got["dw"] = dw.region.detach().cpu()
        o.untouched["dw"] = bool(dw.untouched().all())
        if db is not None:
            o.got["db"] = db.region.detach().cpu()
            o.untouched["db"] = bool(db.untouched().all())
    return o
