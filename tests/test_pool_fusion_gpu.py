"""The encoder level's MaxPool3d(2) folded into its BatchNorm + activation passes (ops.norm_act_pool, mri3d_norm_act_pool_*).

Bars.  The fused operator keeps the expressions, the selection rule and the voxel -> block partition of the two operators it
replaces (ops.norm_act, ops.max_pool3d_skip), so in fp32 every result is BIT-EQUAL to theirs: pooled, skip, running statistics,
dx, dgamma, dbeta, dalpha — and within REL_TOL of a float64 CPU evaluation.  In bf16 the float64 reference rounds the activation
through bf16 before it pools (the stored tensor is what the pool compares); results are held to BF16_TOL = 4 * 2^-8 of the
tensor's largest magnitude — up to three roundings through storage lie between the inputs and dx (activation, summed gradient,
dx itself), half an ulp = 2^-9 each, with a factor of about two for |gamma * invstd * alpha| above one — and may be no further
from the reference than the two-operator path is."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from guard import guarded, kernels_launched
from util import REL_TOL, rel_err, to_ncdhw

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL3D = torch.channels_last_3d
F32, BF = torch.float32, torch.bfloat16
BF16_TOL = 4 * 2.0 ** -8


def _dev(t, dtype=F32):
    return t.to(DEV).to(dtype).contiguous(memory_format=CL3D) if t.dim() == 5 else t.to(DEV)


def _windows(a):
    """(n, c, do, ho, wo, 8): the 2x2x2 windows of a (n, c, d, h, w) tensor, taps in raster order."""
    n, c, d, h, w = a.shape
    return a.reshape(n, c, d // 2, 2, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(n, c, d // 2, h // 2, w // 2, 8)


# (n, c, spatial), statistics, activation, alpha (None, "one", "one-", "each", "each-": per channel, "-" = negative values too),
# dtype, pitched x
CASES = [
    ((1, 4, (2, 2, 2)), "batch", "prelu", "one", F32, False),           # one window, one lane quad
    ((3, 16, (4, 6, 2)), "batch", "prelu", "each-", F32, False),
    ((1, 32, (6, 10, 4)), "running", "relu", None, F32, False),
    ((3, 64, (2, 2, 34)), "none", "leaky_relu", None, F32, False),      # a wave spans rows and samples; four blocks
    ((3, 16, (2, 2, 34)), "batch", "relu", None, F32, False),
    ((1, 64, (2, 8, 34)), "batch", "prelu", "one-", F32, False),        # forward: two h-chunks per slab, the second shorter
    ((3, 16, (6, 10, 4)), "batch", "prelu", "one", F32, True),          # x as channels [4, 20) of a 24-channel buffer; two blocks
    ((3, 32, (6, 10, 4)), "running", "prelu", "each", F32, False),
    ((1, 64, (4, 6, 2)), "batch", "prelu", "each", BF, False),
    ((3, 32, (6, 10, 4)), "batch", "relu", None, BF, False),
    ((1, 4, (2, 2, 34)), "running", "prelu", "one-", BF, False),        # bf16 with 4 channels: 8-byte accesses in the forward
    ((1, 16, (2, 2, 2)), "none", "relu", None, BF, False),
    ((3, 16, (2, 2, 34)), "batch", "prelu", "one", BF, True),
    # n * voxels > 8 * VT * 1024 with VT = 16: the fused operators' block count (nap_plan in csrc/norm.hip) at its cap of 1024,
    # which, unlike norm_plan's, is not divided by the groups
    ((1, 64, (34, 64, 62)), "batch", "prelu", "one", F32, False),
]
IDS = ["%dx%d_%s_%s_%s_%s_%s%s" % (s[0], s[1], "x".join(map(str, s[2])), m, a, al, "bf16" if d == BF else "f32", "_pitched" if p else "")
       for s, m, a, al, d, p in CASES]
ACT = {"prelu": "prelu", "relu": "relu", "leaky_relu": "leaky_relu"}
SLOPE = 0.01


@functools.lru_cache(maxsize=None)
def _inputs(i):
    (n, c, sp), mode, act, al, dtype, _ = CASES[i]
    g = torch.Generator().manual_seed(1000 + i)
    r = lambda *s: torch.randn(*s, generator=g)
    do, ho, wo = (e // 2 for e in sp)
    p = {"x": r(n, c, *sp) * 1.5 + 0.3, "dskip": r(n, c, *sp), "dpool": r(n, c, do, ho, wo),
         "gamma": None, "beta": None, "alpha": None, "rm": None, "rv": None}
    if act == "relu":
        # real ties: whole windows far below zero in every channel, so the activation is an exact zero eight times over
        dead = torch.rand(n, do, ho, wo, generator=g) < 0.3
        dead[0, 0, 0, 0] = True
        dead = dead.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
        p["x"] = torch.where(dead[:, None], -20.0 - p["x"].abs(), p["x"])
    if mode != "none":
        p["gamma"], p["beta"] = 1.0 + 0.2 * r(c), 0.2 * r(c)
        p["rm"], p["rv"] = 0.3 + 0.1 * r(c), 2.0 + 0.3 * torch.rand(c, generator=g)
    if al is not None:
        a = 0.25 + 0.1 * torch.rand(c if al.startswith("each") else 1, generator=g)
        if al.endswith("-"):
            a[::2] = -a[::2]
        p["alpha"] = a
    if dtype == BF:   # the reference sees the values the kernels see
        for k in ("x", "dskip", "dpool"):
            p[k] = p[k].bfloat16().float()
    return p


@functools.lru_cache(maxsize=None)
def _reference(i, grads):
    """float64 CPU: (pooled, skip) and the gradients of sum(pooled * dpool) + sum(skip * dskip), either term optional."""
    (n, c, sp), mode, act, al, dtype, _ = CASES[i]
    p = _inputs(i)
    leaf = {k: (v.double().requires_grad_(True) if v is not None and k in ("x", "gamma", "beta", "alpha") else v) for k, v in p.items()}
    x, bc = leaf["x"], (lambda v: v[None, :, None, None, None])
    if mode == "batch":
        mean, var = x.mean((0, 2, 3, 4)), x.var((0, 2, 3, 4), unbiased=False)
    elif mode == "running":
        mean, var = p["rm"].double(), p["rv"].double()
    u = x if mode == "none" else (x - bc(mean)) / torch.sqrt(bc(var) + 1e-5) * bc(leaf["gamma"]) + bc(leaf["beta"])
    if act == "prelu":
        a_ = leaf["alpha"]
        a = torch.where(u > 0, u, u * (bc(a_) if a_.numel() > 1 else a_))
    elif act == "relu":
        a = torch.relu(u)
    else:
        a = torch.where(u > 0, u, u * SLOPE)
    if dtype == BF:   # the pool compares the stored activation (straight-through for the gradient)
        a = a + (a.detach().float().bfloat16().double() - a.detach())
    pooled = F.max_pool3d(a, 2)
    loss = 0.0
    if grads in ("both", "pool"):
        loss = loss + (pooled * p["dpool"].double()).sum()
    if grads in ("both", "skip"):
        loss = loss + (a * p["dskip"].double()).sum()
    loss.backward()
    res = {"pooled": pooled.detach(), "skip": a.detach()}
    for k in ("x", "gamma", "beta", "alpha"):
        res["d" + k] = leaf[k].grad if leaf[k] is not None else None
    if mode == "batch":   # torch's update: momentum 0.1, unbiased variance
        cnt = x.numel() / x.shape[1]
        res["rm"] = 0.9 * p["rm"].double() + 0.1 * mean.detach()
        res["rv"] = 0.9 * p["rv"].double() + 0.1 * var.detach() * cnt / (cnt - 1)
    w = _windows(a.detach())
    res["tie_share"] = ((w == w.max(-1, keepdim=True).values).sum(-1) > 1).double().mean().item()
    return res


def _run(i, grads, fused):
    from mri_epilepsy_diagnosis_amd import ops
    (n, c, sp), mode, act, al, dtype, pitched = CASES[i]
    p = _inputs(i)
    t = {k: (_dev(v, dtype if k in ("x", "dskip", "dpool") else F32) if v is not None else None) for k, v in p.items()}
    if pitched:
        wide = torch.zeros(n, c + 8, *sp, device=DEV, dtype=dtype).contiguous(memory_format=CL3D)
        wide[:, 4:4 + c] = t["x"]
        t["x"] = wide[:, 4:4 + c]
        assert not t["x"].is_contiguous(memory_format=CL3D)
    for k in ("x", "gamma", "beta", "alpha"):
        if t[k] is not None:
            t[k] = t[k].detach().requires_grad_(True)
    eps = 1e-5 if mode != "none" else 0.0
    if fused:
        assert ops.norm_act_pool_supported(t["x"], 2, None, 0, mode, ACT[act], t["alpha"]), "the predicate declined a listed case"
        fn = lambda: ops.norm_act_pool(t["x"], t["gamma"], t["beta"], t["alpha"], t["rm"], t["rv"], mode, 0.1, eps, ACT[act], SLOPE)
    else:
        fn = lambda: ops.max_pool3d_skip(ops.norm_act(t["x"], t["gamma"], t["beta"], t["alpha"], t["rm"], t["rv"], mode, 0.1, eps,
                                                      ACT[act], SLOPE), 2)
    (pooled, skip), names = kernels_launched(fn)
    assert any("norm_act_pool_fwd_kernel" in k for k in names) == fused, names
    outs, gouts = [], []
    if grads in ("both", "pool"):
        outs.append(pooled), gouts.append(t["dpool"])
    if grads in ("both", "skip"):
        outs.append(skip), gouts.append(t["dskip"])
    _, names = kernels_launched(lambda: torch.autograd.backward(outs, gouts))
    assert any("norm_act_pool_bwd_kernel" in k for k in names) == fused, names
    if fused:
        assert not any(key in k for k in names for key in ("maxpool", "norm_act_bwd_reduce", "norm_act_bwd_apply", "norm_act_bwd_frozen")), names
    res = {"pooled": to_ncdhw(pooled).float(), "skip": to_ncdhw(skip).float(), "rm": t["rm"], "rv": t["rv"]}
    for k in ("x", "gamma", "beta", "alpha"):
        gk = t[k].grad if t[k] is not None else None
        res["d" + k] = None if gk is None else (to_ncdhw(gk).float() if k == "x" else gk.detach().float().cpu())
    return res


@pytest.mark.parametrize("grads", ["both", "skip", "pool"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fused_operator_against_two_operators_and_float64(i, grads):
    (n, c, sp), mode, act, al, dtype, _ = CASES[i]
    p = _inputs(i)
    ref = _reference(i, grads)
    if act == "relu":     # the test's own precondition: the first-maximum rule has ties to decide
        assert ref["tie_share"] > 0.0, ref["tie_share"]
    un = _run(i, grads, fused=False)
    fu = _run(i, grads, fused=True)
    tol = REL_TOL if dtype == F32 else BF16_TOL
    for k in ("pooled", "skip", "dx", "dgamma", "dbeta", "dalpha"):
        assert (fu[k] is None) == (ref[k] is None) == (un[k] is None), k
        if ref[k] is None:
            continue
        ef, eu = rel_err(fu[k], ref[k]), rel_err(un[k], ref[k])
        print("%-7s fused %.3e  two operators %.3e  tolerance %.3e" % (k, ef, eu, tol))
        if dtype == F32:
            assert torch.equal(fu[k], un[k]), "%s moved: max |diff| %.3e" % (k, (fu[k] - un[k]).abs().max().item())
        assert ef <= tol, "%s: %.3e > %.3e" % (k, ef, tol)
        assert ef <= eu, "%s: fused %.3e is further from float64 than the two operators %.3e" % (k, ef, eu)
    if mode == "batch":     # running statistics after the call: the same statistics kernel, so the same bits; and right
        for k in ("rm", "rv"):
            assert torch.equal(fu[k], un[k]), k
            assert rel_err(fu[k], ref[k]) <= REL_TOL, k
    elif mode == "running":
        assert torch.equal(fu["rm"].cpu(), p["rm"]) and torch.equal(fu["rv"].cpu(), p["rv"])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_nan_in_a_window_takes_the_later_nans_index(dtype):
    """Windows holding one NaN, two NaNs (the later one's index wins) and a NaN in front of a larger finite value: pooled, skip
    and dx (whose scatter shows the stored index) are those of the two operators.  Running statistics, so a NaN does
    not reach the other voxels of its channel."""
    from mri_epilepsy_diagnosis_amd import ops
    n, c, sp = 2, 16, (4, 6, 4)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, c, *sp, generator=g)
    nan = float("nan")
    x[0, 3, 0, 0, 1] = nan                              # one NaN: window (0,0,0), tap 1
    x[0, 5, 0, 1, 2], x[0, 5, 1, 0, 3] = nan, nan        # two NaNs in window (0,0,1): taps 2 and 5
    x[1, 7, 2, 4, 0], x[1, 7, 3, 5, 1] = nan, 50.0       # NaN at tap 0, then the window's largest finite value at tap 7
    x[1, 9, 3, 5, 3] = nan                              # the last voxel of the tensor
    dskip, dpool = torch.randn(n, c, *sp, generator=g), torch.randn(n, c, 2, 3, 2, generator=g) + 3.0
    gamma, beta, alpha = 1.0 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g), torch.full((1,), 0.25)
    rm, rv = 0.1 * torch.randn(c, generator=g), 1.0 + torch.rand(c, generator=g)
    res = {}
    for fused in (True, False):
        xd = _dev(x, dtype).requires_grad_(True)
        args = (xd, gamma.to(DEV), beta.to(DEV), alpha.to(DEV), rm.to(DEV), rv.to(DEV), "running", 0.1, 1e-5, "prelu")
        pooled, skip = ops.norm_act_pool(*args) if fused else ops.max_pool3d_skip(ops.norm_act(*args), 2)
        torch.autograd.backward([pooled, skip], [_dev(dpool, dtype), _dev(dskip, dtype)])
        torch.cuda.synchronize()
        res[fused] = (pooled.detach(), skip.detach(), xd.grad)
    for name, a, b in zip(("pooled", "skip", "dx"), res[True], res[False]):
        assert bool(torch.isnan(a).any()), name
        # NaN where the two operators have NaN (sign and payload of a NaN are the compiler's choice), the same bits elsewhere
        assert torch.equal(torch.isnan(a), torch.isnan(b)), name
        assert torch.equal(_bits(torch.nan_to_num(a.float(), nan=0.0)), _bits(torch.nan_to_num(b.float(), nan=0.0))), name
    pooled = to_ncdhw(res[True][0]).float()
    assert bool(torch.isnan(pooled[0, 3, 0, 0, 0])) and bool(torch.isnan(pooled[0, 5, 0, 0, 1])) and bool(torch.isnan(pooled[1, 7, 1, 2, 0]))
    assert int(torch.isnan(pooled).sum()) == 4


def _geoms(n, c, sp, dtype, act, alpha_n, x_ld=None, instance=0, k=2):
    from mri_epilepsy_diagnosis_amd import _lib
    d, h, w = sp
    dt = _lib.BF16 if dtype == BF else _lib.F32
    g = _lib.NormGeom(n, d * h * w, c, c if x_ld is None else x_ld, c, instance, act, alpha_n, 0.0, 1e-5, 0, dt)
    pg = _lib.PoolGeom(n, d, h, w, (d - k) // 2 + 1, (h - k) // 2 + 1, (w - k) // 2 + 1, c, k, k, k, 2, 2, 2, 0, 0, 0, c, c, dt)
    return g, pg


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_buffers_guards_and_exact_workspace(training, dtype):
    """Guard bands around skip, pooled, index bytes, dx and the workspace at exactly the queried size (poisoned with NaN: same
    bits as with a roomy one); one byte less is refused with EWORKSPACE before anything is written; the index bytes are those
    mri3d_maxpool3d_fwd writes for the stored skip tensor."""
    from mri_epilepsy_diagnosis_amd import _lib
    L = _lib.lib()
    n, c, sp = 3, 16, (6, 10, 4)
    do, ho, wo = (e // 2 for e in sp)
    g, pg = _geoms(n, c, sp, dtype, _lib.ACT_PRELU, c)
    need = L.mri3d_norm_act_pool_workspace_bytes(ctypes.byref(g), ctypes.byref(pg))
    assert need > 0 and L.mri3d_norm_act_pool_supported(ctypes.byref(g), ctypes.byref(pg)) == 1
    gen = torch.Generator().manual_seed(3)
    x = _dev(torch.randn(n, c, *sp, generator=gen), dtype)
    dskip, dpool = _dev(torch.randn(n, c, *sp, generator=gen), dtype), _dev(torch.randn(n, c, do, ho, wo, generator=gen), dtype)
    mean, invstd = (0.1 * torch.randn(c, generator=gen)).to(DEV), (0.5 + torch.rand(c, generator=gen)).to(DEV)
    gamma, beta = (1.0 + 0.2 * torch.randn(c, generator=gen)).to(DEV), (0.2 * torch.randn(c, generator=gen)).to(DEV)
    alpha = (0.25 + 0.1 * torch.rand(c, generator=gen)).to(DEV)
    P = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def once(ws_bytes, expect=0):
        skip, pooled = guarded((n, *sp, c), dtype), guarded((n, do, ho, wo, c), dtype)
        idx, dx = guarded(n * do * ho * wo * c, torch.uint8), guarded((n, *sp, c), dtype)
        dg, db, da = (guarded(c, F32) for _ in range(3))
        ws = guarded(ws_bytes, torch.uint8)
        ws.flat[:ws_bytes // 8 * 8].view(torch.float64).fill_(float("nan"))
        _lib.check(L.mri3d_norm_act_pool_fwd(ctypes.byref(g), ctypes.byref(pg), P(x), P(mean), P(invstd), P(gamma), P(beta), P(alpha),
                                             P(skip.region), P(pooled.region), P(idx.region), s), "fwd")
        rc = L.mri3d_norm_act_pool_bwd(ctypes.byref(g), ctypes.byref(pg), training, P(x), P(dskip), P(dpool), P(idx.region), P(mean),
                                       P(invstd), P(gamma), P(beta), P(alpha), P(dx.region), P(dg.region), P(db.region), P(da.region),
                                       P(ws.flat), ws_bytes, s)
        torch.cuda.synchronize()
        assert rc == expect, (rc, L.mri3d_last_error())
        for gd, what in ((skip, "skip"), (pooled, "pooled"), (idx, "index bytes"), (dx, "dx"), (ws, "workspace"), (dg, "dgamma"),
                         (db, "dbeta"), (da, "dalpha")):
            gd.assert_guards_intact(what)
        assert not bool(skip.untouched().any()) and not bool(pooled.untouched().any())
        assert int(idx.region.max()) <= 7
        written = (dx, dg, db, da)
        if expect != 0:       # refused on the host: nothing was written
            assert all(bool(v.untouched().all()) for v in written)
            return None
        assert not any(bool(v.untouched().any()) for v in written)
        # the index bytes of the plain pool over the stored skip tensor
        idx2, y2 = torch.empty_like(idx.region), torch.empty_like(pooled.region)
        _lib.check(L.mri3d_maxpool3d_fwd(ctypes.byref(pg), P(skip.region), P(y2), P(idx2), s), "maxpool3d_fwd")
        torch.cuda.synchronize()
        assert torch.equal(idx2, idx.region) and torch.equal(_bits(y2), _bits(pooled.region))
        return [v.region.clone() for v in (skip, pooled, idx, dx, dg, db, da)]

    roomy = once(need + (1 << 20))
    for a, b in zip(once(need), roomy):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)
    assert once(need - 1, expect=-4) is None


class _OneRank:
    def all_reduce(self, t):
        return t


@pytest.mark.parametrize("what", ["odd extents", "kernel 3", "c = 12", "instance", "sync"])
def test_predicate_declines_and_the_block_keeps_two_operators(what):
    from mri_epilepsy_diagnosis_amd import _lib, nn as mnn, ops
    from mri_epilepsy_diagnosis_amd.unet.unet import EncodingBlock
    L = _lib.lib()
    c, sp, k, norm = 16, (8, 8, 8), 2, "batch"
    if what == "odd extents":
        sp = (8, 7, 8)
    elif what == "kernel 3":
        k = 3
    elif what == "c = 12":
        c = 12
    elif what == "instance":
        norm = "instance"
    mode = {"instance": "instance", "sync": "sync"}.get(what, "batch")
    if what != "sync":      # the native query; the synchronised mode is the caller's to see
        g, pg = _geoms(1, c, sp, F32, _lib.ACT_PRELU, 1, instance=1 if what == "instance" else 0, k=k)
        assert L.mri3d_norm_act_pool_supported(ctypes.byref(g), ctypes.byref(pg)) == 0
        assert L.mri3d_norm_act_pool_workspace_bytes(ctypes.byref(g), ctypes.byref(pg)) == 0
    x = torch.randn(1, c, *sp, device=DEV).contiguous(memory_format=CL3D)
    assert not ops.norm_act_pool_supported(x, k, 2, 0, mode, "prelu", torch.full((1,), 0.25, device=DEV))
    torch.manual_seed(0)
    blk = EncodingBlock(1, c // 2, 3, norm, "max", is_first_block=True, padding=1, activation="PReLU").to(DEV)
    if k != 2:
        blk.downsample = mnn.MaxPool3d(kernel_size=k, stride=2)
    xin = torch.randn(2, 1, *sp, device=DEV)
    prev = ops.set_sync_batchnorm(_OneRank() if what == "sync" else None)
    try:
        (pooled, skip), names = kernels_launched(lambda: blk(xin))
        assert skip.shape == (2, c, *sp) and pooled.shape[2:] == tuple((e - k) // 2 + 1 for e in sp)
        assert not any("norm_act_pool" in n_ for n_ in names), names
        assert any("maxpool" in n_ for n_ in names), names
        p2, s2 = blk(xin, fused_pool=False)      # train mode: the result does not depend on the running statistics
        assert torch.equal(p2, pooled) and torch.equal(s2, skip)
    finally:
        ops.set_sync_batchnorm(prev)
    # and the same block folds the pool when nothing stands in the way
    if what in ("sync",):
        _, names = kernels_launched(lambda: blk(xin))
        assert any("norm_act_pool_fwd_kernel" in n_ for n_ in names), names


def _model(seed=0):
    from mri_epilepsy_diagnosis_amd.unet import UNet
    torch.manual_seed(seed)
    return UNet(in_channels=1, out_classes=2, dimensions=3, num_encoding_blocks=3, out_channels_first_layer=8,
                normalization="batch", upsampling_type="linear", padding=True, activation="PReLU")


def _step_kernel_names(net, x, t):
    from torch.profiler import ProfilerActivity, profile
    from mri_epilepsy_diagnosis_amd import ops
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        logits = net(x)
        loss = ops.softmax_dice_loss(logits, t)
        loss.backward()
        torch.cuda.synchronize()
    return logits.detach(), loss.detach(), [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.mark.parametrize("shape", [(1, 1, 16, 16, 16), (2, 1, 16, 24, 16)])
def test_model_fused_pool_equals_two_operator_tail(shape):
    base = _model()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, generator=g).to(DEV)
    t = (torch.rand(*shape, generator=g) < 0.2).float().to(DEV)
    runs = {}
    for fused in (True, False):
        net = copy.deepcopy(base).to(DEV)
        assert net.fused_pool            # the default
        net.fused_pool = fused
        logits, loss, names = _step_kernel_names(net, x, t)
        runs[fused] = (logits, loss, {k: v.grad for k, v in net.named_parameters()}, dict(net.named_buffers()), names)
    (lf, ff, gf, bf, nf), (lu, fu, gu, bu, nu) = runs[True], runs[False]
    assert torch.equal(lf, lu), "logits"
    assert torch.equal(ff, fu), "loss"
    assert gf.keys() == gu.keys() and bf.keys() == bu.keys()
    for k in gf:
        assert gf[k] is not None and torch.equal(gf[k], gu[k]), k
        assert gf[k].abs().max().item() > 0 or k.endswith("bias"), k
    for k in bf:
        assert torch.equal(bf[k], bu[k]), k
    # launches of one step, by kernel name: the two encoder tails run the fused kernels and nothing of the two operators
    count = lambda names, key: sum(1 for k in names if key in k)
    assert count(nf, "norm_act_pool_fwd_kernel") == 2 and count(nf, "norm_act_pool_bwd_kernel") == 4
    assert count(nu, "norm_act_pool") == 0
    for key in ("maxpool2_fwd_kernel", "maxpool_bwd_kernel"):
        assert count(nf, key) == 0 and count(nu, key) == 2, key
    for key in ("norm_act_bwd_reduce_kernel", "norm_act_bwd_apply_kernel"):
        assert count(nf, key) == count(nu, key) - 2, key
    assert count([k for k in nf if "norm_act_pw" not in k], "norm_act_fwd_kernel") == \
        count([k for k in nu if "norm_act_pw" not in k], "norm_act_fwd_kernel") - 2


def test_captured_step_with_fused_pool_replays_eager_bit_exactly():
    from mri_epilepsy_diagnosis_amd import ops, parallel
    net = _model(3).to(DEV)
    assert net.fused_pool
    flat = parallel.FlatParams(net)
    x = torch.randn(1, 1, 16, 16, 16, device=DEV)
    t = (torch.rand(1, 1, 16, 16, 16, device=DEV) < 0.2).float()
    cap = parallel.CapturedStep(flat, lambda: ops.softmax_dice_loss(net(x), t)).capture()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(state)
    l_g, g_g = cap.run().clone(), flat.grad.clone()
    net.load_state_dict(state)
    l_e = cap._eager().clone()
    assert torch.equal(l_g, l_e) and torch.equal(g_g, flat.grad) and g_g.abs().max().item() > 0
    cap.release()
