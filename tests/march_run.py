"""What the rows of tests/march_cases.py mean: their geometries and the launch plans the library answers for them (host only), their
inputs, their float64 reference with the counted bounds (tests/march_ref.py), and how they run through the raw entry points
mri3d_conv3d_fwd_march / mri3d_conv3d_dgrad_march on guarded device buffers (tests/guard.py)."""
import ctypes

import torch

import march_cases as mc
import march_ref as mr
from mri_epilepsy_diagnosis_amd import _lib, ops
from mri_epilepsy_diagnosis_amd._lib import BF16, F32, PASS_DGRAD, PASS_FWD, ConvGeom

TYPES = {"f32": F32, "bf16": BF16}
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}
PASSES = {"fwd": PASS_FWD, "dgrad": PASS_DGRAD}
EINVAL, ENOTSUP, EWORKSPACE = -1, -2, -4
NAN = float("nan")


def width(row, name):
    dense = {"x": row.split or row.ci, "x2": row.ci - row.split, "y": row.co}[name]
    return row.layout[name][0] if name in row.layout else dense


def off(row, name):
    return row.layout[name][1] if name in row.layout else 0


# ---------------------------------------------------------------------------------------------- geometries and plans
def geom(row, dtype):
    """the ConvGeom the entry points get: x_ld = the pitch of x (of the first tensor of a split operand), y_ld that of y"""
    D, H, W = row.sp
    return ConvGeom(row.n, D, H, W, row.ci, D, H, W, row.co, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, width(row, "x"), width(row, "y"),
                    TYPES[dtype])


def query_geom(row, dtype):
    """the geometry the host queries get: a split operand is asked about as one tensor (x_ld >= ci), as mri3d_conv3d_march_supported"""
    g = geom(row, dtype)
    if row.split:
        g.x_ld = row.ci
    return g


def plan(row, dtype, p):
    """plan numbers of the pass, or None where the plan refuses"""
    try:
        return ops.conv_march_plan(query_geom(row, dtype), PASSES[p], row.stats and p == "fwd")
    except _lib.Mri3dError:
        return None


def plans(row, dtype):
    return {p: plan(row, dtype, p) for p in row.passes}


def declared_mismatches(row, dtype, got):
    """what of the row's declarations `got` (= plans(...)) does not give: plan numbers, and the passes it says are refused"""
    wrong = []
    for p in row.passes:
        if (got[p] is None) != (not mc.runs(row, dtype, p)):
            wrong.append("%s %s %s: declared %s, the plan %s" % (row.id, dtype, p, "served" if mc.runs(row, dtype, p) else "refused",
                                                                "refuses" if got[p] is None else "serves"))
    for p, d in mc.declared(row, dtype).items():
        for f, v in d.items():
            if got.get(p) is not None and got[p][f] != v:
                wrong.append("%s %s %s: declares %s = %d, the plan has %d" % (row.id, dtype, p, f, v, got[p][f]))
    return wrong


# ---------------------------------------------------------------------------------------------- inputs, reference, bounds
def _uniform(shape, g):
    return torch.rand(shape, generator=g) + 0.5          # [0.5, 1.5): a dropped part of a sum cannot cancel


def make_inputs(row, dtype, seed=0):
    """logical NCDHW CPU tensors: activations of the storage type, weights and bias fp32"""
    g = torch.Generator().manual_seed(seed + 31 * len(row.id) + sum(map(ord, row.id)))
    st = TORCH[dtype]
    return {"x": _uniform((row.n, row.ci) + row.sp, g).to(st), "dy": _uniform((row.n, row.co) + row.sp, g).to(st),
            "w": torch.randn((row.co, row.ci, 3, 3, 3), generator=g), "b": torch.randn(row.co, generator=g) if row.bias else None}


def bounds(row, dtype, inp, pl):
    """{name: (float64 reference, elementwise bound)} of the passes that run; pl = plans(row, dtype)"""
    out = {}
    w = mr.stored_weights(inp["w"], dtype)
    if mc.runs(row, dtype, "fwd"):
        y, A, a, A0 = mr.forward(inp["x"].double(), w, inp["b"].double() if inp["b"] is not None else None)
        out["y"] = (y, mr.stored_bound(y, A, row.ci, dtype))
        if row.stats:
            out["stats"] = mr.stats(a, A0, row.ci, pl["fwd"]["seglen"], pl["fwd"]["grid"])
    if mc.runs(row, dtype, "dgrad"):
        dx, L1 = mr.dgrad(inp["dy"].double(), w, (row.n, row.ci) + row.sp)
        out["dx"] = (dx, mr.stored_bound(dx, L1, row.co, dtype))
    return out


def report(bnd, got):
    """[(name, worst error / bound, elements over)]: every element of every result"""
    assert set(bnd) == set(got), (sorted(bnd), sorted(got))
    return [(k,) + mr.compare(want, b, got[k]) for k, (want, b) in bnd.items()]


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


class Outputs:
    """the guarded buffers of one run, the return codes and the results on the host"""

    def __init__(self):
        self.slices, self.flat, self.got, self.rcs, self.untouched = [], [], {}, {}, {}

    def check(self, what):
        for name, ss in self.slices:
            ss.assert_outside_intact("%s: %s" % (what, name))
        for name, g in self.flat:
            g.assert_guards_intact("%s: %s" % (what, name))


def run(row, dtype, inp, device="cuda", g=None, passes=None, base_shift=0, ws_bytes=None, blocks=None):
    """The row's passes through the raw entry points -> Outputs.  For the refusal tests: g: a geometry to pass instead of the row's;
    passes: instead of those the plan serves; base_shift: elements to move the base of the input by; ws_bytes: the workspace size to state
    instead of the true one; blocks: statistics blocks to allocate where the library names none."""
    import guard
    L = _lib.lib()
    own = geom(row, dtype)
    g = g if g is not None else own
    st = TORCH[dtype]
    c1 = row.split or row.ci
    o = Outputs()
    w = inp["w"].to(device).contiguous()
    esz = torch.empty((), dtype=st).element_size()

    def shifted(t):
        return ctypes.c_void_p(t.data_ptr() + base_shift * esz)

    def workspace(p):
        nbytes = int(L.mri3d_conv3d_workspace_bytes(ctypes.byref(own), PASSES[p]))
        ws = guard.guarded(max(nbytes // 4, 64), torch.float32, device=device)
        o.flat.append(("workspace " + p, ws))
        return ws, (nbytes if ws_bytes is None else ws_bytes)

    todo = passes if passes is not None else [p for p in row.passes if mc.runs(row, dtype, p)]
    if "fwd" in todo:
        x = _input(inp["x"][:, :c1], width(row, "x"), off(row, "x"), device)
        x2 = _input(inp["x"][:, c1:], width(row, "x2"), off(row, "x2"), device) if row.split else None
        b = inp["b"].to(device).contiguous() if inp["b"] is not None else None
        y = guard.SentinelSlice(row.n, width(row, "y"), row.sp, st, off(row, "y"), row.co, device=device)
        o.slices.append(("y", y))
        part = None
        if row.stats:
            nb = blocks if blocks is not None else int(L.mri3d_conv3d_march_stats_blocks(ctypes.byref(query_geom(row, dtype))))
            part = guard.guarded((max(nb, 1), row.co, 2), torch.float64, device=device)      # the sentinel is a NaN
            o.flat.append(("stat_partials", part))
        ws, wsb = workspace("fwd")
        o.rcs["fwd"] = L.mri3d_conv3d_fwd_march(ctypes.byref(g), shifted(x), _p(x2), row.split, width(row, "x2") if row.split else 0,
                                                _p(w), _p(b), _p(y.slice), _p(part.flat) if part is not None else None, _p(ws.flat),
                                                wsb, _stream())
        torch.cuda.synchronize()
        o.got["y"] = y.slice.detach().cpu().contiguous()
        o.untouched["y"] = bool(y.slice_untouched().all())
        if part is not None:
            o.got["stats"] = part.region.cpu().sum(0)
            o.untouched["stats"] = bool(part.untouched().all())
    if "dgrad" in todo:
        dy = _input(inp["dy"], width(row, "y"), off(row, "y"), device)
        dx = guard.SentinelSlice(row.n, width(row, "x"), row.sp, st, off(row, "x"), c1, device=device)
        o.slices.append(("dx", dx))
        dx2 = guard.SentinelSlice(row.n, width(row, "x2"), row.sp, st, off(row, "x2"), row.ci - c1, device=device) if row.split else None
        if dx2 is not None:
            o.slices.append(("dx2", dx2))
        ws, wsb = workspace("dgrad")
        o.rcs["dgrad"] = L.mri3d_conv3d_dgrad_march(ctypes.byref(g), shifted(dy), _p(w), _p(dx.slice), _p(dx2.slice) if dx2 is not None else None,
                                                    row.split, width(row, "x2") if row.split else 0, _p(ws.flat), wsb, _stream())
        torch.cuda.synchronize()
        parts = [dx.slice.detach().cpu()] + ([dx2.slice.detach().cpu()] if dx2 is not None else [])
        o.got["dx"] = torch.cat(parts, 1).contiguous()
        o.untouched["dx"] = bool(dx.slice_untouched().all()) and (dx2 is None or bool(dx2.slice_untouched().all()))
    return o
