"""The case table of the norm-activation parity tests (tests/test_norm_parity_gpu.py), each row with the launch plan it exists for.

`norm_plan()` in csrc/norm.hip decides, per pass, the channels per lane (vec 8 / 4 / 1), the lanes and voxel rows of a block (CL, VT),
the channel chunks (cy), the blocks per group (nblk) and the groups from the channel count, the pitches, the pointers' alignment,
the voxel count and the statistics mode.  A row is there for one corner of that decision; `PLANS[(row id, dtype)][pass]` is the
(vec, CL, VT, cy, nblk, groups) the row was written for.  The decision is a host query (`ops.norm_plan` -> mri3d_norm_plan_query),
so tests/test_norm_plan.py checks on the CPU that every row still gets its plan and that every corner a sweep of the query finds
has a row, and the GPU test asserts the same plans with the real tensors before it launches anything.

Layout of a row: x, the destination (`out=(buffer, offset)`) and the incoming gradient dy are each dense, or channels
[off, off + c) of an NDHWC buffer of `C` channels, written (C, off).  The backward reads a dense copy of a pitched x and writes a
dense dx, so its plan sees the pitch and alignment of dy alone.

Plan arithmetic: lanes = c / vec, CL = min(lanes, 256), VT = 256 / CL, cy = ceil(lanes / CL), want = ceil(gvox / (8 * VT)),
cap = 1024 / (groups * cy) clamped to at least 1, nblk = min(want, cap)."""
import numpy as np
import torch

import norm_ref as nr
from mri_epilepsy_diagnosis_amd import _lib, ops
from mri_epilepsy_diagnosis_amd._lib import BF16, F32, NORM_PASS_BWD, NORM_PASS_FWD, NORM_PASS_STATS

DTYPES = {"f32": F32, "bf16": BF16}
TORCH_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
ESIZE = {"f32": 4, "bf16": 2}
PASSES = {"stats": NORM_PASS_STATS, "fwd": NORM_PASS_FWD, "bwd": NORM_PASS_BWD}
ACT_CODES = {None: _lib.ACT_NONE, "relu": _lib.ACT_RELU, "leaky_relu": _lib.ACT_LEAKY, "prelu": _lib.ACT_PRELU}
TRAINING = ("batch", "instance", "group")
MAX_BLOCKS = 1024          # kNormMaxBlocks
SLOPE, EPS, MOMENTUM = 0.01, 1e-5, 0.1


class Row:
    def __init__(self, rid, mode, act, alpha_n, n, c, sp, x=None, out=None, dy=None, grads=True, group_c=0, data=None,
                 dtypes=("f32", "bf16"), why="", affine=None):
        self.id, self.mode, self.act, self.alpha_n, self.n, self.c, self.sp = rid, mode, act, alpha_n, n, c, tuple(sp)
        self.x, self.out, self.dy, self.grads, self.group_c, self.data, self.dtypes, self.why = x, out, dy, grads, group_c, data, dtypes, why
        self.vox = int(np.prod(sp))
        self.affine = mode != "none" if affine is None else affine      # gamma and beta given
        assert n * c * self.vox <= 10_000_000, rid
        for lay in (x, out, dy):
            assert lay is None or lay[1] + c <= lay[0], rid

    def __repr__(self):
        return self.id

    def passes(self):
        return (("stats",) if self.mode in TRAINING else ()) + ("fwd", "bwd")


def align_of(byte_offset):
    bits = 16 | int(byte_offset)
    return bits & -bits


def _ld(lay, c):
    return c if lay is None else lay[0]


def _al(lay, dtype):
    return 16 if lay is None else align_of(lay[1] * ESIZE[dtype])


def geometry(row, dtype, x_ld, y_ld):
    return _lib.NormGeom(row.n, row.vox, row.c, x_ld, y_ld, 1 if row.mode in ("instance", "group") else 0, ACT_CODES[row.act],
                         row.alpha_n if row.act == "prelu" else 1, SLOPE, EPS, row.group_c if row.mode == "group" else 0, DTYPES[dtype])


def plans(row, dtype, x_align=None, y_align=None, dy_align=None):
    """{pass: (vec, CL, VT, cy, nblk, groups)} of the row as its GPU test runs it.  The alignments default to those of channel
    slices of freshly allocated buffers; the test passes `ops._ptr_align` of its real tensors."""
    c = row.c
    xa = _al(row.x, dtype) if x_align is None else x_align
    ya = _al(row.out, dtype) if y_align is None else y_align
    da = _al(row.dy, dtype) if dy_align is None else dy_align
    x_ld, y_ld, dy_ld = _ld(row.x, c), _ld(row.out, c), _ld(row.dy, c)
    got = {}
    if row.mode in TRAINING:
        got["stats"] = ops.norm_plan(geometry(row, dtype, x_ld, x_ld), NORM_PASS_STATS, xa)[:6]
    got["fwd"] = ops.norm_plan(geometry(row, dtype, x_ld, y_ld), NORM_PASS_FWD, min(xa, ya))[:6]
    # backward: a pitched x is read through a dense copy, dx is a fresh dense tensor
    xb = xa if row.x is None else 16
    got["bwd"] = ops.norm_plan(geometry(row, dtype, c, dy_ld), NORM_PASS_BWD, min(xb, da))[:6]
    return got


def check(row, dtype, x=None, y=None, dy=None):
    """Assert the plans the row declares; with the test's real tensors the query sees their actual base addresses."""
    got = plans(row, dtype, None if x is None else ops._ptr_align(x), None if y is None else ops._ptr_align(y),
                None if dy is None else ops._ptr_align(dy))
    want = PLANS[(row.id, dtype)]
    assert sorted(want) == sorted(got), (row.id, dtype, sorted(want), sorted(got))
    wrong = ["%s %s %s: norm_plan gives (vec, CL, VT, cy, nblk, groups) = %s, the row is there for %s" % (row.id, dtype, p, got[p], want[p])
             for p in got if tuple(got[p]) != tuple(want[p])]
    assert not wrong, "\n  ".join(wrong)
    return got


def block_class(plan, gvox):
    """Why the pass has its block count: "clamped" (groups * cy exceeds the block budget: one block per group and chunk whatever
    the volume), "capped" (the budget cut the count), "1" (one block is enough), "between"."""
    vec, cl, vt, cy, nblk, groups = plan
    want = -(-gvox // (8 * vt))
    raw = MAX_BLOCKS // (groups * cy)
    if raw < 1:
        return "clamped"
    if want > raw:
        return "capped"
    return "1" if nblk == 1 else "between"


def corner(pass_, dtype, c, plan, gvox):
    """The corner of the plan space a pass of a geometry sits in: what the completeness sweep collects and the rows claim."""
    vec, cl, vt, cy, nblk, groups = plan
    return (pass_, dtype, vec, cl == c // vec, 256 % cl == 0, cy > 1, block_class(plan, gvox))


def corners(row, dtype):
    gvox = row.vox if row.mode in ("instance", "group") else row.n * row.vox
    return {corner(p, dtype, row.c, pl, gvox) for p, pl in plans(row, dtype).items()}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_inputs(row, dtype):
    """The row's inputs on the CPU, deterministic: dict with x, dy (storage dtype, logical NCDHW), gamma, beta, alpha, rm, rv
    (fp32, None where the row has none) and `conditioning` = (rounds, elements changed) of norm_ref.condition, which x has been
    through."""
    seed = 1000 + 7 * [r.id for r in ROWS].index(row.id)
    n, c, sp = row.n, row.c, row.sp
    bf16 = dtype == "bf16"
    shape = (n, c) + sp
    if row.data == "offset":      # mean / std about 6000
        x = torch.randn(shape, generator=_gen(seed)) * 0.05 + 300.0
    else:
        x = torch.randn(shape, generator=_gen(seed)) * 1.7 + 0.9
    if row.data == "const":       # one channel without variance
        x[:, 1] = 0.5
    g = _gen(seed + 2)
    sign = torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0)
    gamma = sign * (0.5 + torch.rand(c, generator=g)) if row.affine else None
    beta = torch.randn(c, generator=g) * 0.3 if row.affine else None
    if row.data == "offset":      # keeps the share of elements near the kink, whose width grows with |mean|, below 1 %
        beta = torch.full((c,), 2.5) + torch.randn(c, generator=g) * 0.1
    if row.data == "const":
        beta[1] = 0.3
    alpha = (torch.rand(row.alpha_n, generator=g) * 0.5 - 0.1) if row.act == "prelu" else None
    rm = torch.randn(c, generator=g) * 0.1 + 0.8 if row.mode in ("batch", "running") else None
    rv = torch.rand(c, generator=g) + 2.0 if row.mode in ("batch", "running") else None
    x64 = nr.round_bf16(x) if bf16 else x.double()
    running = (rm, rv) if row.mode == "running" else None
    x64, rounds, changed = nr.condition(x64, gamma, beta, row.mode, row.act, EPS, row.group_c, running, bf16=bf16)
    # The incoming gradient has a mean and a share along sign(gamma) * xhat (the direction of the pre-activation), so that
    # S0 = sum du and S1 = sum du * xhat are of the size of their L1 sums on either side of the activation: the dx bound is stated
    # relative to |k1| ~ |S0| and |k2| ~ |S1|, while the rounding errors of the sums grow with the L1 sums.  A gradient whose sums
    # cancel (pure noise over a handful of voxels) puts a correct kernel outside that bound.
    mean, _, invstd, _ = nr.statistics(x64, row.mode, EPS, row.group_c, running)
    along = (x64 - mean) * invstd * (torch.sign(gamma).double().reshape(1, c, 1, 1, 1) if gamma is not None else 1.0)
    dy = (0.25 * torch.randn(shape, generator=_gen(seed + 1)).double() + 0.6 + 0.4 * along).float()
    dy64 = nr.round_bf16(dy) if bf16 else dy.double()
    td = TORCH_DTYPES[dtype]
    xs, dys = x64.to(td), dy64.to(td)
    assert torch.equal(xs.double(), x64) and torch.equal(dys.double(), dy64)
    return dict(x=xs, dy=dys, gamma=gamma, beta=beta, alpha=alpha, rm=rm, rv=rv, conditioning=(rounds, changed))


def reference(row, dtype, inp):
    running = (inp["rm"], inp["rv"]) if inp["rm"] is not None else None
    return nr.norm_act_ref(inp["x"].double(), inp["dy"].double(), inp["gamma"], inp["beta"], inp["alpha"], row.mode, row.act, SLOPE, EPS,
                           row.group_c, running, MOMENTUM, bf16=dtype == "bf16")


def _slice_of(lay, shape, dtype, device):
    """A zero-filled NDHWC buffer of lay[0] channels and its channel slice [lay[1], lay[1] + c)."""
    n, c = shape[:2]
    buf = torch.zeros((n, lay[0]) + tuple(shape[2:]), dtype=dtype, device=device).contiguous(memory_format=torch.channels_last_3d)
    return buf.narrow(1, lay[1], c)


def run_row(row, dtype, inp, device="cuda", plan_check=True):
    """One forward + backward of the row through ops.norm_act on fresh device tensors laid out as the row says; the declared
    plans are asserted with those tensors before anything is launched.  Returns (results, SentinelSlice or None): results holds y,
    dx, dgamma, dbeta, dalpha, running_mean, running_var as device tensors, None where the row has none."""
    from guard import SentinelSlice
    td = TORCH_DTYPES[dtype]
    shape = tuple(inp["x"].shape)
    cl = torch.channels_last_3d
    if row.x is None:
        xd = inp["x"].to(device).contiguous(memory_format=cl)
    else:
        xd = _slice_of(row.x, shape, td, device)
        xd.copy_(inp["x"])
        xd = xd.detach()
    xd.requires_grad_(True)
    if row.dy is None:
        dyd = inp["dy"].to(device).contiguous(memory_format=cl)
    else:
        dyd = _slice_of(row.dy, shape, td, device)
        dyd.copy_(inp["dy"])
    ss = SentinelSlice(row.n, row.out[0], row.sp, td, row.out[1], row.c, device=device) if row.out is not None else None
    par = [None if t is None else t.to(device).requires_grad_(row.grads) for t in (inp["gamma"], inp["beta"], inp["alpha"])]
    gd, bd, ad = par
    rm = inp["rm"].to(device) if inp["rm"] is not None else None
    rv = inp["rv"].to(device) if inp["rv"] is not None else None
    if plan_check:
        check(row, dtype, x=xd, y=None if ss is None else ss.slice, dy=dyd)
    y = ops.norm_act(xd, gd, bd, ad, rm, rv, row.mode, MOMENTUM, EPS, row.act, SLOPE, None if ss is None else (ss.buf, ss.off), row.group_c)
    wanted = [t for t in par if t is not None and row.grads]
    grads = list(torch.autograd.grad(y, [xd] + wanted, dyd))
    res = dict(y=y.detach(), dx=grads.pop(0), dgamma=None, dbeta=None, dalpha=None, running_mean=None, running_var=None)
    for name, t in zip(("dgamma", "dbeta", "dalpha"), par):
        if t is not None and row.grads:
            res[name] = grads.pop(0)
    if row.mode == "batch":
        res["running_mean"], res["running_var"] = rm, rv
    return res, ss


def cpu_fp32(row, inp):
    """The same forward + backward in torch's own fp32 CPU operators (what the older tests compare with): y, dx, dgamma, dbeta,
    dalpha as float64 tensors, for the diagnostic that sets the kernel's error next to torch's."""
    import torch.nn.functional as F
    x = inp["x"].float().clone().requires_grad_(True)
    par = [None if t is None else t.clone().requires_grad_(True) for t in (inp["gamma"], inp["beta"], inp["alpha"])]
    g, b, a = par
    if row.mode == "batch":
        t = F.batch_norm(x, None, None, g, b, True, MOMENTUM, EPS)
    elif row.mode == "running":
        t = F.batch_norm(x, inp["rm"].clone(), inp["rv"].clone(), g, b, False, MOMENTUM, EPS)
    elif row.mode == "instance":
        t = F.instance_norm(x, None, None, g, b, True, MOMENTUM, EPS)
    elif row.mode == "group":
        t = F.group_norm(x, row.c // row.group_c, g, b, EPS)
    else:
        t = x
    y = {None: lambda v: v, "relu": F.relu, "leaky_relu": lambda v: F.leaky_relu(v, SLOPE), "prelu": lambda v: F.prelu(v, a)}[row.act](t)
    wanted = [p for p in par if p is not None and (p is not a or row.act == "prelu")]
    grads = list(torch.autograd.grad(y, [x] + wanted, inp["dy"].float()))
    res = dict(y=y.detach().double(), dx=grads.pop(0).double(), dgamma=None, dbeta=None, dalpha=None)
    for name, p in zip(("dgamma", "dbeta", "dalpha"), par):
        if p is not None and (p is not a or row.act == "prelu"):
            res[name] = grads.pop(0).double()
    return res


SMALL = (3, 5, 7)        # n = 2: 210 voxels per channel
MID = (8, 8, 10)         # n = 2: 1280
MIS16 = dict(x=(20, 2), dy=(20, 2))      # c = 16 with x and dy off a 4-element boundary: vec 1 in every pass

ROWS = [
    # ---- vector width: what forces vec = 1, on each of the three tensors (one block, 16 channels unless the count is the cause)
    Row("vw_dense16", "batch", "prelu", 1, 2, 16, SMALL, why="vec 4 dense baseline; bf16 forward: vec 8"),
    Row("vw_c7", "batch", "prelu", 1, 2, 7, SMALL, why="vec 1: c % 4 != 0; 7 lanes do not divide 256"),
    Row("vw_x_pitch", "batch", "prelu", 1, 2, 16, SMALL, x=(18, 0), why="vec 1 by the pitch of x, pointer 16-byte aligned"),
    Row("vw_x_ptr", "batch", "prelu", 1, 2, 16, SMALL, x=(20, 2), why="vec 1 by the pointer of x, pitch a multiple of 4"),
    Row("vw_out_pitch", "batch", "prelu", 1, 2, 16, SMALL, out=(18, 0), why="forward vec 1 by the pitch of the destination"),
    Row("vw_out_ptr", "batch", "prelu", 1, 2, 16, SMALL, out=(20, 2), why="forward vec 1 by the pointer of the destination"),
    Row("vw_dy_pitch", "batch", "prelu", 1, 2, 16, SMALL, dy=(18, 0), why="backward vec 1 by the pitch of dy, x dense"),
    Row("vw_dy_ptr", "batch", "prelu", 1, 2, 16, SMALL, dy=(20, 2), why="backward vec 1 by the pointer of dy, x dense"),
    # ---- bf16 forward width: 8 -> 4 -> 1 (statistics and backward stay at vec <= 4)
    Row("w4_c12", "batch", "relu", 1, 2, 12, SMALL, why="bf16 forward vec 4: c % 8 != 0; 3 lanes (VT 85)"),
    Row("w4_pitch20", "batch", "prelu", 16, 2, 16, SMALL, x=(20, 0), why="bf16 forward vec 4: pitch 20"),
    Row("w4_off8B", "batch", "prelu", 16, 2, 16, SMALL, x=(24, 4), why="bf16 forward vec 4: 8-byte but not 16-byte aligned offset"),
    Row("w1_off4B", "batch", "prelu", 16, 2, 16, SMALL, x=(24, 2), why="bf16 vec 1: 4-byte aligned offset"),
    # ---- lane counts that do not divide 256, one per statistics mode (c = 12: w4_c12)
    Row("lanes_c20_instance", "instance", "leaky_relu", 1, 3, 20, SMALL, why="5 lanes, VT 51"),
    Row("lanes_c24_group", "group", "relu", 1, 3, 24, SMALL, group_c=6, why="6 lanes, VT 42; GroupNorm with parameter gradients, 4 groups"),
    Row("lanes_c40_running", "running", "prelu", 40, 2, 40, SMALL, why="10 lanes, VT 25; frozen backward with parameter gradients"),
    Row("lanes_c48_none", "none", "prelu", 48, 2, 48, SMALL, why="12 lanes, VT 21; activation only, dalpha from the one-pass kernel"),
    # ---- more than 256 lanes: cy = 2, per-channel slopes so that the parameter block loops over c > blockDim
    Row("wide_c1028", "batch", "prelu", 1028, 1, 1028, (2, 3, 5), why="vec 4, cy 2, second chunk one lane"),
    Row("wide_c260_mis", "batch", "prelu", 260, 1, 260, (2, 3, 5), x=(264, 2), dy=(264, 2), why="vec 1, cy 2"),
    Row("wide_c1028_one", "batch", "prelu", 1028, 1, 1028, (1, 2, 3), why="vec 4, cy 2, one block per chunk"),
    Row("wide_c260_mis_one", "batch", "prelu", 260, 1, 260, (1, 2, 3), x=(264, 2), dy=(264, 2), why="vec 1, cy 2, one block per chunk"),
    Row("wide_c1028_capped", "instance", "prelu", 1028, 257, 1028, (1, 3, 3), why="vec 4, cy 2, cap 1 < want 2"),
    Row("wide_c260_mis_capped", "instance", "prelu", 260, 257, 260, (1, 3, 3), x=(264, 2), dy=(264, 2), why="vec 1, cy 2, cap 1 < want 2"),
    Row("wide_c1028_clamped", "instance", "prelu", 1028, 513, 1028, (2, 2, 2), why="vec 4, groups * cy = 1026 blocks"),
    Row("wide_c260_mis_clamped", "instance", "prelu", 260, 513, 260, (2, 2, 2), x=(264, 2), dy=(264, 2), why="vec 1, groups * cy = 1026 blocks"),
    # ---- block count, vec 4 (bf16 forward: 8), lanes dividing 256
    Row("blk_between", "batch", "prelu", 1, 2, 16, MID, why="1 < nblk < cap"),
    Row("blk_cap_c64_dense", "batch", "prelu", 1, 1, 64, (34, 64, 62), dtypes=("f32",), why="cap 1024 reached, groups 1, VT 16"),
    Row("blk_cap_inst513_c16", "instance", "leaky_relu", 1, 513, 16, (5, 5, 41), dtypes=("bf16",), why="bf16 forward vec 8 capped (cap 1)"),
    Row("blk_clamp_n1030_c4", "instance", "prelu", 1, 1030, 4, (2, 2, 2), why="cap < 1 clamped to 1: groups * nblk = 1030 > 1024"),
    Row("blk_clamp_n1030_c8", "instance", "relu", 1, 1030, 8, (2, 2, 2), why="bf16 forward vec 8, clamped"),
    Row("blk_between_c4", "batch", "prelu", 4, 2, 4, (5, 5, 41), why="one lane (VT 256), want 2; bf16 forward stays at vec 4"),
    Row("blk_cap_inst513_c4", "instance", "prelu", 1, 513, 4, (3, 683, 1), dtypes=("bf16",), why="bf16 forward vec 4 capped (cap 1), one lane"),
    # ---- block count, vec 4, 3 lanes
    Row("blk_between_c12", "batch", "prelu", 12, 2, 12, (8, 8, 12), why="VT 85, want 3"),
    Row("blk_cap_inst513_c12", "instance", "relu", 1, 513, 12, (3, 227, 1), why="VT 85, cap 1 < want 2"),
    Row("blk_clamp_n1030_c12", "instance", "prelu", 12, 1030, 12, (2, 2, 2), why="VT 85, clamped"),
    # ---- block count, bf16 forward vec 8 with 3 lanes
    Row("blk_one_c24", "batch", "prelu", 1, 2, 24, SMALL, why="bf16 forward vec 8, 3 lanes, one block"),
    Row("blk_between_c24", "batch", "leaky_relu", 1, 2, 24, (8, 8, 12), why="bf16 forward vec 8, 3 lanes, want 3"),
    Row("blk_cap_inst513_c24", "instance", "relu", 1, 513, 24, (3, 227, 1), dtypes=("bf16",), why="bf16 forward vec 8, 3 lanes, capped"),
    Row("blk_clamp_n1030_c24", "instance", "prelu", 1, 1030, 24, (2, 2, 2), why="bf16 forward vec 8, 3 lanes, clamped"),
    # ---- block count, vec 1, 16 lanes
    Row("blk1_one", "batch", "prelu", 1, 2, 16, (3, 3, 7), why="vec 1, VT 16, one block", **MIS16),
    Row("blk1_between", "batch", "prelu", 16, 2, 16, MID, why="vec 1, VT 16, want 10", **MIS16),
    Row("blk_cap_c256_mis", "batch", "prelu", 256, 1, 256, (17, 22, 22), x=(260, 2), dy=(260, 2), why="cap 1024 reached, groups 1, VT 1"),
    Row("blk_cap_inst40", "instance", "leaky_relu", 1, 40, 16, (15, 15, 15), why="instance mode, cap 25 reached", **MIS16),
    Row("blk1_clamp_n1030_c2", "instance", "prelu", 2, 1030, 2, (2, 2, 2), why="vec 1, 2 lanes, clamped"),
    # ---- block count, vec 1, 7 and 3 lanes
    Row("blk1_between_c7", "batch", "relu", 1, 2, 7, MID, why="vec 1, VT 36, want 5"),
    Row("blk1_cap_inst513_c7", "instance", "prelu", 7, 513, 7, (17, 17, 1), why="vec 1, VT 36, cap 1 < want 2"),
    Row("blk1_clamp_n1030_c3", "instance", "leaky_relu", 1, 1030, 3, (2, 2, 2), why="vec 1, 3 lanes, clamped"),
    # ---- loop remainders: one block, VT 64; a thread takes 5 or 4 rows (261 voxels), 3 or 2 rows (158): every residue mod 4 of the
    # statistics loop and both parities of the backward loops, body and tail, and the row counts differ inside the block
    Row("rem_261", "batch", "prelu", 1, 1, 16, (1, 9, 29), why="5 and 4 rows per thread"),
    Row("rem_158", "batch", "prelu", 16, 1, 16, (1, 2, 79), why="3 and 2 rows per thread"),
    # ---- backward launch sequences (training with every gradient: the rows above)
    Row("bwd_train_nograds", "batch", "prelu", 1, 2, 16, SMALL, grads=False, why="training, no parameter gradient wanted: dx alone"),
    Row("bwd_running_nograds", "running", "prelu", 16, 2, 16, SMALL, grads=False, why="frozen, none wanted: the apply kernel alone"),
    Row("bwd_none_nograds", "none", "leaky_relu", 1, 2, 16, SMALL, grads=False, why="activation only, none wanted"),
    Row("gn_nograds", "group", "prelu", 1, 3, 8, SMALL, group_c=2, grads=False, why="GroupNorm without parameter gradients"),
    Row("gn_one_group", "group", "prelu", 6, 3, 6, SMALL, group_c=6, why="GroupNorm, group_c = c"),
    Row("gn_gc1", "group", "leaky_relu", 1, 3, 8, SMALL, group_c=1, why="GroupNorm, group_c = 1"),
    Row("gn_three_groups", "group", "prelu", 1, 3, 12, SMALL, group_c=4, why="GroupNorm, 3 groups"),
    # ---- conditioning of the statistics
    Row("off_batch", "batch", "leaky_relu", 1, 2, 8, (8, 8, 8), data="offset", dtypes=("f32",), why="mean / std about 6000"),
    Row("off_instance", "instance", "leaky_relu", 1, 2, 8, (8, 8, 8), data="offset", dtypes=("f32",), why="mean / std about 6000"),
    Row("off_group", "group", "leaky_relu", 1, 2, 8, (8, 8, 8), group_c=4, data="offset", dtypes=("f32",), why="mean / std about 6000"),
    Row("const_channel", "batch", "prelu", 8, 2, 8, SMALL, data="const", why="a channel whose values are all equal"),
    # ---- mean and invstd themselves: identity activation, no affine parameters, y = (x - mean) * invstd
    Row("ident_batch", "batch", None, 1, 2, 8, SMALL, why="statistics observable through y", affine=False),
    Row("ident_instance", "instance", None, 1, 3, 8, SMALL, why="statistics observable through y", affine=False),
    Row("ident_group", "group", None, 1, 3, 8, SMALL, group_c=4, why="statistics observable through y", affine=False),
]
assert len({r.id for r in ROWS}) == len(ROWS)
BY_ID = {r.id: r for r in ROWS}
PAIRS = [(r, dt) for r in ROWS for dt in r.dtypes]
PAIR_IDS = ["%s-%s" % (r.id, dt) for r, dt in PAIRS]
# the rows whose exact-size, poisoned workspace tests/test_buffer_contracts_gpu.py checks: groups * nblk > kNormMaxBlocks
WS_ROWS = ("blk_clamp_n1030_c4",)

# (row id, dtype) -> {pass: (vec, CL, VT, cy, nblk, groups)}: what each row is there for
PLANS = {
    ("vw_dense16", "f32"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (4, 4, 64, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("vw_dense16", "bf16"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (8, 2, 128, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("vw_c7", "f32"): {"stats": (1, 7, 36, 1, 1, 1), "fwd": (1, 7, 36, 1, 1, 1), "bwd": (1, 7, 36, 1, 1, 1)},
    ("vw_c7", "bf16"): {"stats": (1, 7, 36, 1, 1, 1), "fwd": (1, 7, 36, 1, 1, 1), "bwd": (1, 7, 36, 1, 1, 1)},
    ("vw_x_pitch", "f32"): {"stats": (1, 16, 16, 1, 2, 1), "fwd": (1, 16, 16, 1, 2, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("vw_x_pitch", "bf16"): {"stats": (1, 16, 16, 1, 2, 1), "fwd": (1, 16, 16, 1, 2, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("vw_x_ptr", "f32"): {"stats": (1, 16, 16, 1, 2, 1), "fwd": (1, 16, 16, 1, 2, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("vw_x_ptr", "bf16"): {"stats": (1, 16, 16, 1, 2, 1), "fwd": (1, 16, 16, 1, 2, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("vw_out_pitch", "f32"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (1, 16, 16, 1, 2, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("vw_out_pitch", "bf16"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (1, 16, 16, 1, 2, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("vw_out_ptr", "f32"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (1, 16, 16, 1, 2, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("vw_out_ptr", "bf16"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (1, 16, 16, 1, 2, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("vw_dy_pitch", "f32"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (4, 4, 64, 1, 1, 1), "bwd": (1, 16, 16, 1, 2, 1)},
    ("vw_dy_pitch", "bf16"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (8, 2, 128, 1, 1, 1), "bwd": (1, 16, 16, 1, 2, 1)},
    ("vw_dy_ptr", "f32"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (4, 4, 64, 1, 1, 1), "bwd": (1, 16, 16, 1, 2, 1)},
    ("vw_dy_ptr", "bf16"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (8, 2, 128, 1, 1, 1), "bwd": (1, 16, 16, 1, 2, 1)},
    ("w4_c12", "f32"): {"stats": (4, 3, 85, 1, 1, 1), "fwd": (4, 3, 85, 1, 1, 1), "bwd": (4, 3, 85, 1, 1, 1)},
    ("w4_c12", "bf16"): {"stats": (4, 3, 85, 1, 1, 1), "fwd": (4, 3, 85, 1, 1, 1), "bwd": (4, 3, 85, 1, 1, 1)},
    ("w4_pitch20", "f32"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (4, 4, 64, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("w4_pitch20", "bf16"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (4, 4, 64, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("w4_off8B", "f32"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (4, 4, 64, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("w4_off8B", "bf16"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (4, 4, 64, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("w1_off4B", "f32"): {"stats": (1, 16, 16, 1, 2, 1), "fwd": (1, 16, 16, 1, 2, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("w1_off4B", "bf16"): {"stats": (1, 16, 16, 1, 2, 1), "fwd": (1, 16, 16, 1, 2, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("lanes_c20_instance", "f32"): {"stats": (4, 5, 51, 1, 1, 3), "fwd": (4, 5, 51, 1, 1, 3), "bwd": (4, 5, 51, 1, 1, 3)},
    ("lanes_c20_instance", "bf16"): {"stats": (4, 5, 51, 1, 1, 3), "fwd": (4, 5, 51, 1, 1, 3), "bwd": (4, 5, 51, 1, 1, 3)},
    ("lanes_c24_group", "f32"): {"stats": (4, 6, 42, 1, 1, 3), "fwd": (4, 6, 42, 1, 1, 3), "bwd": (4, 6, 42, 1, 1, 3)},
    ("lanes_c24_group", "bf16"): {"stats": (4, 6, 42, 1, 1, 3), "fwd": (8, 3, 85, 1, 1, 3), "bwd": (4, 6, 42, 1, 1, 3)},
    ("lanes_c40_running", "f32"): {"fwd": (4, 10, 25, 1, 2, 1), "bwd": (4, 10, 25, 1, 2, 1)},
    ("lanes_c40_running", "bf16"): {"fwd": (8, 5, 51, 1, 1, 1), "bwd": (4, 10, 25, 1, 2, 1)},
    ("lanes_c48_none", "f32"): {"fwd": (4, 12, 21, 1, 2, 1), "bwd": (4, 12, 21, 1, 2, 1)},
    ("lanes_c48_none", "bf16"): {"fwd": (8, 6, 42, 1, 1, 1), "bwd": (4, 12, 21, 1, 2, 1)},
    ("wide_c1028", "f32"): {"stats": (4, 256, 1, 2, 4, 1), "fwd": (4, 256, 1, 2, 4, 1), "bwd": (4, 256, 1, 2, 4, 1)},
    ("wide_c1028", "bf16"): {"stats": (4, 256, 1, 2, 4, 1), "fwd": (4, 256, 1, 2, 4, 1), "bwd": (4, 256, 1, 2, 4, 1)},
    ("wide_c260_mis", "f32"): {"stats": (1, 256, 1, 2, 4, 1), "fwd": (1, 256, 1, 2, 4, 1), "bwd": (1, 256, 1, 2, 4, 1)},
    ("wide_c260_mis", "bf16"): {"stats": (1, 256, 1, 2, 4, 1), "fwd": (1, 256, 1, 2, 4, 1), "bwd": (1, 256, 1, 2, 4, 1)},
    ("wide_c1028_one", "f32"): {"stats": (4, 256, 1, 2, 1, 1), "fwd": (4, 256, 1, 2, 1, 1), "bwd": (4, 256, 1, 2, 1, 1)},
    ("wide_c1028_one", "bf16"): {"stats": (4, 256, 1, 2, 1, 1), "fwd": (4, 256, 1, 2, 1, 1), "bwd": (4, 256, 1, 2, 1, 1)},
    ("wide_c260_mis_one", "f32"): {"stats": (1, 256, 1, 2, 1, 1), "fwd": (1, 256, 1, 2, 1, 1), "bwd": (1, 256, 1, 2, 1, 1)},
    ("wide_c260_mis_one", "bf16"): {"stats": (1, 256, 1, 2, 1, 1), "fwd": (1, 256, 1, 2, 1, 1), "bwd": (1, 256, 1, 2, 1, 1)},
    ("wide_c1028_capped", "f32"): {"stats": (4, 256, 1, 2, 1, 257), "fwd": (4, 256, 1, 2, 1, 257), "bwd": (4, 256, 1, 2, 1, 257)},
    ("wide_c1028_capped", "bf16"): {"stats": (4, 256, 1, 2, 1, 257), "fwd": (4, 256, 1, 2, 1, 257), "bwd": (4, 256, 1, 2, 1, 257)},
    ("wide_c260_mis_capped", "f32"): {"stats": (1, 256, 1, 2, 1, 257), "fwd": (1, 256, 1, 2, 1, 257), "bwd": (1, 256, 1, 2, 1, 257)},
    ("wide_c260_mis_capped", "bf16"): {"stats": (1, 256, 1, 2, 1, 257), "fwd": (1, 256, 1, 2, 1, 257), "bwd": (1, 256, 1, 2, 1, 257)},
    ("wide_c1028_clamped", "f32"): {"stats": (4, 256, 1, 2, 1, 513), "fwd": (4, 256, 1, 2, 1, 513), "bwd": (4, 256, 1, 2, 1, 513)},
    ("wide_c1028_clamped", "bf16"): {"stats": (4, 256, 1, 2, 1, 513), "fwd": (4, 256, 1, 2, 1, 513), "bwd": (4, 256, 1, 2, 1, 513)},
    ("wide_c260_mis_clamped", "f32"): {"stats": (1, 256, 1, 2, 1, 513), "fwd": (1, 256, 1, 2, 1, 513), "bwd": (1, 256, 1, 2, 1, 513)},
    ("wide_c260_mis_clamped", "bf16"): {"stats": (1, 256, 1, 2, 1, 513), "fwd": (1, 256, 1, 2, 1, 513), "bwd": (1, 256, 1, 2, 1, 513)},
    ("blk_between", "f32"): {"stats": (4, 4, 64, 1, 3, 1), "fwd": (4, 4, 64, 1, 3, 1), "bwd": (4, 4, 64, 1, 3, 1)},
    ("blk_between", "bf16"): {"stats": (4, 4, 64, 1, 3, 1), "fwd": (8, 2, 128, 1, 2, 1), "bwd": (4, 4, 64, 1, 3, 1)},
    ("blk_cap_c64_dense", "f32"): {"stats": (4, 16, 16, 1, 1024, 1), "fwd": (4, 16, 16, 1, 1024, 1), "bwd": (4, 16, 16, 1, 1024, 1)},
    ("blk_cap_inst513_c16", "bf16"): {"stats": (4, 4, 64, 1, 1, 513), "fwd": (8, 2, 128, 1, 1, 513), "bwd": (4, 4, 64, 1, 1, 513)},
    ("blk_clamp_n1030_c4", "f32"): {"stats": (4, 1, 256, 1, 1, 1030), "fwd": (4, 1, 256, 1, 1, 1030), "bwd": (4, 1, 256, 1, 1, 1030)},
    ("blk_clamp_n1030_c4", "bf16"): {"stats": (4, 1, 256, 1, 1, 1030), "fwd": (4, 1, 256, 1, 1, 1030), "bwd": (4, 1, 256, 1, 1, 1030)},
    ("blk_clamp_n1030_c8", "f32"): {"stats": (4, 2, 128, 1, 1, 1030), "fwd": (4, 2, 128, 1, 1, 1030), "bwd": (4, 2, 128, 1, 1, 1030)},
    ("blk_clamp_n1030_c8", "bf16"): {"stats": (4, 2, 128, 1, 1, 1030), "fwd": (8, 1, 256, 1, 1, 1030), "bwd": (4, 2, 128, 1, 1, 1030)},
    ("blk_between_c4", "f32"): {"stats": (4, 1, 256, 1, 2, 1), "fwd": (4, 1, 256, 1, 2, 1), "bwd": (4, 1, 256, 1, 2, 1)},
    ("blk_between_c4", "bf16"): {"stats": (4, 1, 256, 1, 2, 1), "fwd": (4, 1, 256, 1, 2, 1), "bwd": (4, 1, 256, 1, 2, 1)},
    ("blk_cap_inst513_c4", "bf16"): {"stats": (4, 1, 256, 1, 1, 513), "fwd": (4, 1, 256, 1, 1, 513), "bwd": (4, 1, 256, 1, 1, 513)},
    ("blk_between_c12", "f32"): {"stats": (4, 3, 85, 1, 3, 1), "fwd": (4, 3, 85, 1, 3, 1), "bwd": (4, 3, 85, 1, 3, 1)},
    ("blk_between_c12", "bf16"): {"stats": (4, 3, 85, 1, 3, 1), "fwd": (4, 3, 85, 1, 3, 1), "bwd": (4, 3, 85, 1, 3, 1)},
    ("blk_cap_inst513_c12", "f32"): {"stats": (4, 3, 85, 1, 1, 513), "fwd": (4, 3, 85, 1, 1, 513), "bwd": (4, 3, 85, 1, 1, 513)},
    ("blk_cap_inst513_c12", "bf16"): {"stats": (4, 3, 85, 1, 1, 513), "fwd": (4, 3, 85, 1, 1, 513), "bwd": (4, 3, 85, 1, 1, 513)},
    ("blk_clamp_n1030_c12", "f32"): {"stats": (4, 3, 85, 1, 1, 1030), "fwd": (4, 3, 85, 1, 1, 1030), "bwd": (4, 3, 85, 1, 1, 1030)},
    ("blk_clamp_n1030_c12", "bf16"): {"stats": (4, 3, 85, 1, 1, 1030), "fwd": (4, 3, 85, 1, 1, 1030), "bwd": (4, 3, 85, 1, 1, 1030)},
    ("blk_one_c24", "f32"): {"stats": (4, 6, 42, 1, 1, 1), "fwd": (4, 6, 42, 1, 1, 1), "bwd": (4, 6, 42, 1, 1, 1)},
    ("blk_one_c24", "bf16"): {"stats": (4, 6, 42, 1, 1, 1), "fwd": (8, 3, 85, 1, 1, 1), "bwd": (4, 6, 42, 1, 1, 1)},
    ("blk_between_c24", "f32"): {"stats": (4, 6, 42, 1, 5, 1), "fwd": (4, 6, 42, 1, 5, 1), "bwd": (4, 6, 42, 1, 5, 1)},
    ("blk_between_c24", "bf16"): {"stats": (4, 6, 42, 1, 5, 1), "fwd": (8, 3, 85, 1, 3, 1), "bwd": (4, 6, 42, 1, 5, 1)},
    ("blk_cap_inst513_c24", "bf16"): {"stats": (4, 6, 42, 1, 1, 513), "fwd": (8, 3, 85, 1, 1, 513), "bwd": (4, 6, 42, 1, 1, 513)},
    ("blk_clamp_n1030_c24", "f32"): {"stats": (4, 6, 42, 1, 1, 1030), "fwd": (4, 6, 42, 1, 1, 1030), "bwd": (4, 6, 42, 1, 1, 1030)},
    ("blk_clamp_n1030_c24", "bf16"): {"stats": (4, 6, 42, 1, 1, 1030), "fwd": (8, 3, 85, 1, 1, 1030), "bwd": (4, 6, 42, 1, 1, 1030)},
    ("blk1_one", "f32"): {"stats": (1, 16, 16, 1, 1, 1), "fwd": (1, 16, 16, 1, 1, 1), "bwd": (1, 16, 16, 1, 1, 1)},
    ("blk1_one", "bf16"): {"stats": (1, 16, 16, 1, 1, 1), "fwd": (1, 16, 16, 1, 1, 1), "bwd": (1, 16, 16, 1, 1, 1)},
    ("blk1_between", "f32"): {"stats": (1, 16, 16, 1, 10, 1), "fwd": (1, 16, 16, 1, 10, 1), "bwd": (1, 16, 16, 1, 10, 1)},
    ("blk1_between", "bf16"): {"stats": (1, 16, 16, 1, 10, 1), "fwd": (1, 16, 16, 1, 10, 1), "bwd": (1, 16, 16, 1, 10, 1)},
    ("blk_cap_c256_mis", "f32"): {"stats": (1, 256, 1, 1, 1024, 1), "fwd": (1, 256, 1, 1, 1024, 1), "bwd": (1, 256, 1, 1, 1024, 1)},
    ("blk_cap_c256_mis", "bf16"): {"stats": (1, 256, 1, 1, 1024, 1), "fwd": (1, 256, 1, 1, 1024, 1), "bwd": (1, 256, 1, 1, 1024, 1)},
    ("blk_cap_inst40", "f32"): {"stats": (1, 16, 16, 1, 25, 40), "fwd": (1, 16, 16, 1, 25, 40), "bwd": (1, 16, 16, 1, 25, 40)},
    ("blk_cap_inst40", "bf16"): {"stats": (1, 16, 16, 1, 25, 40), "fwd": (1, 16, 16, 1, 25, 40), "bwd": (1, 16, 16, 1, 25, 40)},
    ("blk1_clamp_n1030_c2", "f32"): {"stats": (1, 2, 128, 1, 1, 1030), "fwd": (1, 2, 128, 1, 1, 1030), "bwd": (1, 2, 128, 1, 1, 1030)},
    ("blk1_clamp_n1030_c2", "bf16"): {"stats": (1, 2, 128, 1, 1, 1030), "fwd": (1, 2, 128, 1, 1, 1030), "bwd": (1, 2, 128, 1, 1, 1030)},
    ("blk1_between_c7", "f32"): {"stats": (1, 7, 36, 1, 5, 1), "fwd": (1, 7, 36, 1, 5, 1), "bwd": (1, 7, 36, 1, 5, 1)},
    ("blk1_between_c7", "bf16"): {"stats": (1, 7, 36, 1, 5, 1), "fwd": (1, 7, 36, 1, 5, 1), "bwd": (1, 7, 36, 1, 5, 1)},
    ("blk1_cap_inst513_c7", "f32"): {"stats": (1, 7, 36, 1, 1, 513), "fwd": (1, 7, 36, 1, 1, 513), "bwd": (1, 7, 36, 1, 1, 513)},
    ("blk1_cap_inst513_c7", "bf16"): {"stats": (1, 7, 36, 1, 1, 513), "fwd": (1, 7, 36, 1, 1, 513), "bwd": (1, 7, 36, 1, 1, 513)},
    ("blk1_clamp_n1030_c3", "f32"): {"stats": (1, 3, 85, 1, 1, 1030), "fwd": (1, 3, 85, 1, 1, 1030), "bwd": (1, 3, 85, 1, 1, 1030)},
    ("blk1_clamp_n1030_c3", "bf16"): {"stats": (1, 3, 85, 1, 1, 1030), "fwd": (1, 3, 85, 1, 1, 1030), "bwd": (1, 3, 85, 1, 1, 1030)},
    ("rem_261", "f32"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (4, 4, 64, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("rem_261", "bf16"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (8, 2, 128, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("rem_158", "f32"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (4, 4, 64, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("rem_158", "bf16"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (8, 2, 128, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("bwd_train_nograds", "f32"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (4, 4, 64, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("bwd_train_nograds", "bf16"): {"stats": (4, 4, 64, 1, 1, 1), "fwd": (8, 2, 128, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("bwd_running_nograds", "f32"): {"fwd": (4, 4, 64, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("bwd_running_nograds", "bf16"): {"fwd": (8, 2, 128, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("bwd_none_nograds", "f32"): {"fwd": (4, 4, 64, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("bwd_none_nograds", "bf16"): {"fwd": (8, 2, 128, 1, 1, 1), "bwd": (4, 4, 64, 1, 1, 1)},
    ("gn_nograds", "f32"): {"stats": (4, 2, 128, 1, 1, 3), "fwd": (4, 2, 128, 1, 1, 3), "bwd": (4, 2, 128, 1, 1, 3)},
    ("gn_nograds", "bf16"): {"stats": (4, 2, 128, 1, 1, 3), "fwd": (8, 1, 256, 1, 1, 3), "bwd": (4, 2, 128, 1, 1, 3)},
    ("gn_one_group", "f32"): {"stats": (1, 6, 42, 1, 1, 3), "fwd": (1, 6, 42, 1, 1, 3), "bwd": (1, 6, 42, 1, 1, 3)},
    ("gn_one_group", "bf16"): {"stats": (1, 6, 42, 1, 1, 3), "fwd": (1, 6, 42, 1, 1, 3), "bwd": (1, 6, 42, 1, 1, 3)},
    ("gn_gc1", "f32"): {"stats": (4, 2, 128, 1, 1, 3), "fwd": (4, 2, 128, 1, 1, 3), "bwd": (4, 2, 128, 1, 1, 3)},
    ("gn_gc1", "bf16"): {"stats": (4, 2, 128, 1, 1, 3), "fwd": (8, 1, 256, 1, 1, 3), "bwd": (4, 2, 128, 1, 1, 3)},
    ("gn_three_groups", "f32"): {"stats": (4, 3, 85, 1, 1, 3), "fwd": (4, 3, 85, 1, 1, 3), "bwd": (4, 3, 85, 1, 1, 3)},
    ("gn_three_groups", "bf16"): {"stats": (4, 3, 85, 1, 1, 3), "fwd": (4, 3, 85, 1, 1, 3), "bwd": (4, 3, 85, 1, 1, 3)},
    ("off_batch", "f32"): {"stats": (4, 2, 128, 1, 1, 1), "fwd": (4, 2, 128, 1, 1, 1), "bwd": (4, 2, 128, 1, 1, 1)},
    ("off_instance", "f32"): {"stats": (4, 2, 128, 1, 1, 2), "fwd": (4, 2, 128, 1, 1, 2), "bwd": (4, 2, 128, 1, 1, 2)},
    ("off_group", "f32"): {"stats": (4, 2, 128, 1, 1, 2), "fwd": (4, 2, 128, 1, 1, 2), "bwd": (4, 2, 128, 1, 1, 2)},
    ("const_channel", "f32"): {"stats": (4, 2, 128, 1, 1, 1), "fwd": (4, 2, 128, 1, 1, 1), "bwd": (4, 2, 128, 1, 1, 1)},
    ("const_channel", "bf16"): {"stats": (4, 2, 128, 1, 1, 1), "fwd": (8, 1, 256, 1, 1, 1), "bwd": (4, 2, 128, 1, 1, 1)},
    ("ident_batch", "f32"): {"stats": (4, 2, 128, 1, 1, 1), "fwd": (4, 2, 128, 1, 1, 1), "bwd": (4, 2, 128, 1, 1, 1)},
    ("ident_batch", "bf16"): {"stats": (4, 2, 128, 1, 1, 1), "fwd": (8, 1, 256, 1, 1, 1), "bwd": (4, 2, 128, 1, 1, 1)},
    ("ident_instance", "f32"): {"stats": (4, 2, 128, 1, 1, 3), "fwd": (4, 2, 128, 1, 1, 3), "bwd": (4, 2, 128, 1, 1, 3)},
    ("ident_instance", "bf16"): {"stats": (4, 2, 128, 1, 1, 3), "fwd": (8, 1, 256, 1, 1, 3), "bwd": (4, 2, 128, 1, 1, 3)},
    ("ident_group", "f32"): {"stats": (4, 2, 128, 1, 1, 3), "fwd": (4, 2, 128, 1, 1, 3), "bwd": (4, 2, 128, 1, 1, 3)},
    ("ident_group", "bf16"): {"stats": (4, 2, 128, 1, 1, 3), "fwd": (8, 1, 256, 1, 1, 3), "bwd": (4, 2, 128, 1, 1, 3)},
}
