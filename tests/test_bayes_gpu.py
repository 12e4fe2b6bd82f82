"""GPU parity suite of BayesConv3d and the variational-dropout U-Net: the kernels of csrc/bayes.hip, `ops.bayes_conv3d`,
`nn.BayesConv3d` and segmentation/models/bayes_unet.py against tests/bayes_ref.py in float64, always with the SAME injected
noise (the operator takes its noise as an input, so every comparison here is deterministic)."""
import functools

import numpy as np
import pytest
import torch

import bayes_ref
import guard
from util import REL_TOL, load_golden, rel_err, seeded_randn, to_ncdhw

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL3D = torch.channels_last_3d
BF = torch.bfloat16
EDGES = (-5.0, 3.0, 5.0)      # the clamp's two ends and the eval-mode threshold


def _ops():
    from mri_epilepsy_diagnosis_amd import ops
    return ops


# ----------------------------------------------------------------------------------------------- weights: draw and nudge
def _raw64(mu, ls):
    return ls.double() - torch.log(mu.double() ** 2 + 1e-8)


@functools.lru_cache(maxsize=None)
def draw_weights(shape, seed):
    """mu ~ N(0, 0.05) with one exact 0 and one 1e-4, logsigma ~ U(-14, -1); any element whose float64 raw lies within 1e-3 of
    -5, 3 or 5 gets logsigma += 0.01, so that no fp32 rounding of raw can change the side of a clamp end or of the threshold it
    is on.  Asserts (CPU) that none remains that close and that at most 1 % were moved.  Returns CPU fp32 (mu, logsigma)."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(shape, generator=g) * 0.05
    mu.view(-1)[0], mu.view(-1)[1] = 0.0, 1e-4
    ls = torch.rand(shape, generator=g) * 13 - 14

    def near(raw):
        return functools.reduce(torch.logical_or, [(raw - e).abs() < 1e-3 for e in EDGES])
    moved = near(_raw64(mu, ls))
    ls[moved] += 0.01
    assert not near(_raw64(mu, ls)).any()
    assert moved.float().mean().item() <= 0.01, int(moved.sum())
    return mu, ls


def _weights_ref(mu, ls, evaluate, ups):
    """float64 autograd of the formula: outputs and (dmu, dlogsigma) for the upstream gradients `ups` = (g_mean, g_var, g_alpha)."""
    mu64, ls64 = mu.double().requires_grad_(), ls.double().requires_grad_()
    w_mean, w_var, log_alpha = bayes_ref.weight_transform(mu64, ls64, not evaluate, 3)
    loss = (w_mean * ups[0].double()).sum() + (w_var * ups[1].double()).sum() + (log_alpha * ups[2].double()).sum()
    dmu, dls = torch.autograd.grad(loss, (mu64, ls64))
    return w_mean.detach(), w_var.detach(), log_alpha.detach(), dmu, dls


@pytest.mark.parametrize("evaluate", [False, True], ids=["train", "eval"])
@pytest.mark.parametrize("seed", [0, 1])
def test_weight_kernels_match_float64_autograd(seed, evaluate):
    """Bar 1e-5 (max-norm relative, per tensor): a handful of fp32 operations at <= 2 ulp each and |raw| <= 19 in front of the
    exponential give about 1e-6; times ten."""
    ops = _ops()
    shape = (16, 8, 27)
    mu, ls = draw_weights(shape, seed)
    raw = _raw64(mu, ls)
    for lo, hi in ((-1e9, -5), (-5, 3), (3, 5), (5, 1e9)):      # every regime of the formula is populated
        frac = ((raw > lo) & (raw < hi)).float().mean().item()
        assert frac >= 0.05, (lo, hi, frac)
    g = torch.Generator().manual_seed(100 + seed)
    ups = [torch.randn(shape, generator=g) for _ in range(3)]
    ref_mean, ref_var, ref_alpha, ref_dmu, ref_dls = _weights_ref(mu, ls, evaluate, ups)

    mu_d, ls_d = mu.to(DEV).requires_grad_(), ls.to(DEV).requires_grad_()
    outs = ops._BayesWeightsFn.apply(mu_d, ls_d, evaluate, 3)
    w_mean, w_var, log_alpha = outs if evaluate else (mu_d,) + tuple(outs)
    loss = sum((o * u.to(DEV)).sum() for o, u in zip((w_mean, w_var, log_alpha), ups))
    dmu, dls = torch.autograd.grad(loss, (mu_d, ls_d))
    got = {"w_var": (w_var, ref_var), "log_alpha": (log_alpha, ref_alpha), "dmu": (dmu, ref_dmu), "dlogsigma": (dls, ref_dls)}
    if evaluate:
        got["w_mean"] = (w_mean, ref_mean)
        masked = (ref_alpha >= 3)
        assert masked.any() and not masked.all()
        assert (w_mean.detach().cpu()[masked] == 0).all() and (w_var.detach().cpu()[masked] == 0).all()   # exactly zero
        assert torch.equal(w_mean.detach().cpu()[~masked], mu[~masked])
    for name, (a, b) in got.items():
        assert torch.isfinite(a).all(), name
        e = rel_err(a, b)
        print("weights %s seed %d %s: rel err %.3e" % ("eval" if evaluate else "train", seed, name, e))
        assert e <= 1e-5, (name, e)
    # log_alpha alone (a KL term and nothing else): the gradient still reaches both parameters
    mu_d.grad = ls_d.grad = None
    outs = ops._BayesWeightsFn.apply(mu_d, ls_d, evaluate, 3)
    (outs[-1] * ups[2].to(DEV)).sum().backward()
    zero = torch.zeros(shape)
    r = _weights_ref(mu, ls, evaluate, [zero, zero, ups[2]])
    assert rel_err(mu_d.grad, r[3]) <= 1e-5 and rel_err(ls_d.grad, r[4]) <= 1e-5


# ----------------------------------------------------------------------------------------------- operator, fp32
# (n, ci, co, (d, h, w), k, stride, pad, bias, mode)
ROUTE_VOLUME = (1, 369, 161)   # see test_route_case_is_the_smallest_tiled_volume
CASES = [
    (2, 8, 16, (6, 10, 12), 3, 1, 1, True, "train"),
    (1, 1, 4, (8, 8, 8), 3, 1, 1, False, "train"),          # first layer: x needs no gradient
    (1, 6, 10, (5, 7, 9), 3, 2, 1, True, "train"),          # stride 2, odd extents, scalar path of the streaming kernels
    (2, 8, 8, (4, 6, 8), 1, 1, 0, True, "eval"),
    (1, 16, 16, ROUTE_VOLUME, 3, 1, 1, False, "train"),     # the tiled 3x3x3 MFMA kernel instead of the direct one
]
IDS = ["8-16-k3-train", "first-layer", "6-10-s2-odd", "8-8-k1-eval", "16-16-tiled"]


def test_route_case_is_the_smallest_tiled_volume():
    """CASES[4] is the smallest single 16 -> 16 volume the route query sends to a tiled or marching 3x3x3 kernel (found by asking
    `ops.conv3d_routes` on the host for every (d, h, w) with extents below 400 in order of voxel count); spot-check the claim
    around it."""
    ops = _ops()

    def fwd(vol):
        return ops.conv3d_routes((1, 16) + tuple(vol), (16, 16, 3, 3, 3), 1, 1, 1, bias=False)
    r = fwd(ROUTE_VOLUME)
    assert r["fwd"].split()[0] in ("tiled", "march") and r["dgrad"].split()[0] in ("tiled", "march"), r
    d, h, w = ROUTE_VOLUME
    for smaller in ((d, h - 1, w), (d, h, w - 1), (3, 123, 160), (39, 39, 39), (8, 64, 116)):
        assert np.prod(smaller) < d * h * w and fwd(smaller)["fwd"].startswith("direct"), smaller


def _case_tensors(case, seed=0):
    n, ci, co, vol, k, stride, pad, bias, mode = case
    mu, ls = draw_weights((co, ci, k, k, k), seed + 10)
    g = torch.Generator().manual_seed(seed + 20)
    t = {"mu": mu, "ls": ls, "x": torch.randn(n, ci, *vol, generator=g)}
    t["mb"] = (torch.rand(co, generator=g) * 0.4 - 0.2) if bias else None
    t["lb"] = (torch.rand(co, generator=g) * 0.4 - 0.2) if bias else None
    out = tuple((i + 2 * pad - k) // stride + 1 for i in vol)
    t["eps"] = torch.randn(n, co, *out, generator=g)
    t["gy"] = torch.randn(n, co, *out, generator=g)
    t["ga"] = torch.randn(co, ci, k, k, k, generator=g)
    return t


def _reference(case, t, dtype=torch.float64):
    """float64 restatement: the tensors of `_names` for the loss sum(y gy) + sum(log_alpha ga)."""
    n, ci, co, vol, k, stride, pad, bias, mode = case
    leaf = {key: (None if t[key] is None else t[key].to(dtype).requires_grad_()) for key in ("x", "mu", "ls", "mb", "lb")}
    y, la = bayes_ref.bayes_conv3d(leaf["x"], leaf["mu"], leaf["ls"], leaf["mb"], leaf["lb"], stride, pad, 1, mode == "train", 3,
                                   t["eps"].to(dtype))
    ((y * t["gy"].to(dtype)).sum() + (la * t["ga"].to(dtype)).sum()).backward()
    res = {"y": y.detach(), "log_alpha": la.detach(), "dx": leaf["x"].grad, "dmu_weight": leaf["mu"].grad, "dlogsigma_weight": leaf["ls"].grad}
    if bias:
        res.update(dmu_bias=leaf["mb"].grad, dlogsigma_bias=leaf["lb"].grad)
    return res


def _product(case, t, x_dev=None, cast=False, first_layer=False):
    """One forward + backward of ops.bayes_conv3d on the device -> the same dict (dx None when x took no gradient)."""
    ops = _ops()
    n, ci, co, vol, k, stride, pad, bias, mode = case
    x = (t["x"].to(DEV).contiguous(memory_format=CL3D) if x_dev is None else x_dev).detach().requires_grad_(not first_layer)
    p = {key: (None if t[key] is None else t[key].to(DEV).requires_grad_()) for key in ("mu", "ls", "mb", "lb")}
    eps = t["eps"].to(DEV)
    ctx = ops.autocast() if cast else ops.autocast(enabled=False)
    with ctx:
        y, la = ops.bayes_conv3d(x, p["mu"], p["ls"], p["mb"], p["lb"], stride, pad, 1, mode == "train", 3, eps)
    ((y.float() * t["gy"].to(DEV)).sum() + (la * t["ga"].to(DEV)).sum()).backward()
    res = {"y": y.detach(), "log_alpha": la.detach(), "dx": x.grad, "dmu_weight": p["mu"].grad, "dlogsigma_weight": p["ls"].grad}
    if bias:
        res.update(dmu_bias=p["mb"].grad, dlogsigma_bias=p["lb"].grad)
    return res


def _same_bits(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bayes_conv3d_fp32_matches_float64_restatement(case):
    t = _case_tensors(case)
    first = case[1] == 1
    ref = _reference(case, t)
    got = _product(case, t, first_layer=first)
    assert got["y"].is_contiguous(memory_format=CL3D) and got["y"].dtype == torch.float32
    if first:
        assert got["dx"] is None                  # the two data gradients were skipped
        ref.pop("dx"), got.pop("dx")
    for name in ref:
        e = rel_err(to_ncdhw(got[name]) if got[name].dim() == 5 else got[name], ref[name])
        print("%s %s: rel err %.3e" % (IDS[CASES.index(case)], name, e))
        assert torch.isfinite(got[name]).all(), name
        assert e <= REL_TOL, (name, e)
    again = _product(case, t, first_layer=first)
    assert _same_bits(got, again), "two runs differ"


def test_bayes_conv3d_reads_a_channel_slice_and_leaves_the_buffer_alone():
    """x = channels [8, 16) of a 24-channel NDHWC buffer full of sentinels: same results bit for bit as from a dense x, and no other
    channel of the buffer changes."""
    case = CASES[0]
    t = _case_tensors(case)
    n, ci, co, vol = case[:4]
    s = guard.SentinelSlice(n, 24, vol, torch.float32, 8, ci)
    s.slice.copy_(t["x"].to(DEV))
    assert _ops()._pitch_of(s.slice) == 24
    got = _product(case, t, x_dev=s.slice)
    torch.cuda.synchronize()
    s.assert_outside_intact("bayes_conv3d input slice")
    assert torch.equal(s.slice, t["x"].to(DEV))
    dense = _product(case, t)
    assert _same_bits(got, dense)


def test_bayes_conv3d_argument_errors():
    ops = _ops()
    x = torch.zeros(1, 4, 4, 4, 4, device=DEV)
    w = torch.zeros(4, 4, 3, 3, 3, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.bayes_conv3d(x, w, w, padding="same")
    with pytest.raises(NotImplementedError):
        ops.bayes_conv3d(x, w, w, groups=2)
    with pytest.raises(RuntimeError, match="eps has shape"):
        ops.bayes_conv3d(x, w, w, padding=1, eps=torch.zeros(1, 4, 2, 2, 2, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bayes_conv3d(x.cpu(), w, w)


def test_default_noise_is_standard_normal_and_follows_the_generator():
    """eps=None: float32 standard normals from torch's device generator, drawn in y's NDHWC order — with mu = 0 and a constant
    variance the output IS the noise (times a constant)."""
    ops = _ops()
    x = torch.ones(2, 4, 8, 8, 8, device=DEV)
    mu = torch.zeros(6, 4, 1, 1, 1, device=DEV)
    ls = torch.full((6, 4, 1, 1, 1), -5.0, device=DEV)
    lb = torch.full((6,), 2.0, device=DEV)        # var_out = logsigma_bias^2 = 4 everywhere (mu = 0 gives w_var = 0)
    torch.manual_seed(5)
    y1, _ = ops.bayes_conv3d(x, mu, ls, torch.zeros(6, device=DEV), lb)
    torch.manual_seed(5)
    want = torch.empty(2, 8, 8, 8, 6, device=DEV).normal_().permute(0, 4, 1, 2, 3) * float(np.sqrt(np.float32(1e-4) + np.float32(4.0)))
    y2, _ = ops.bayes_conv3d(x, mu, ls, torch.zeros(6, device=DEV), lb)
    assert not torch.equal(y1, y2)                                      # the generator moved on
    assert rel_err(y1, want) <= 1e-6
    z = y1 / 2.0
    assert abs(z.mean().item()) < 0.1 and abs(z.std().item() - 1.0) < 0.1


# ----------------------------------------------------------------------------------------------- guard bands
def _fill(region, c, seed, positive=False):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(region.shape[:-1] + (c,), generator=g)
    region[..., :c] = (v.abs() if positive else v).to(region.device).to(region.dtype)
    return region[..., :c].float()


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c,ld", [(6, 6), (6, 8), (8, 8), (16, 24)])
def test_volume_kernels_stay_inside_guard_bands(c, ld, dtype):
    """C = 6 at pitch 6 (dense) and 8 (a slice): the scalar path; C = 8 dense and C = 16 at pitch 24: 16 bytes per lane.  5x7x9
    voxels.  Each kernel writes every element of its C channels, nothing in the pitch gap, nothing in the guards — out of place and,
    where the ABI allows it, in place."""
    from mri_epilepsy_diagnosis_amd import _lib
    L = _lib.lib()
    ops = _ops()
    nvox = 5 * 7 * 9
    dt = _lib.BF16 if dtype == BF else _lib.F32
    st, P = ops._stream(), ops._ptr
    tol = 2.0 ** -7 if dtype == BF else 1e-6

    def src(seed, positive=False):      # an input tensor of pitch ld (gap channels hold the sentinel, which is a NaN)
        gd = guard.guarded((nvox, ld), dtype)
        return gd, _fill(gd.region, c, seed, positive)

    def check(gd, want, what, in_place=False):
        torch.cuda.synchronize()
        gd.assert_guards_intact(what)
        un = gd.untouched()
        assert un[:, c:].all(), what + ": pitch gap written"
        if not in_place:
            assert not un[:, :c].any(), what + ": elements left unwritten"
        got = gd.region[:, :c].float()
        assert torch.isfinite(got).all() and rel_err(got, want) <= tol, (what, rel_err(got, want))

    eps = guard.guarded((nvox, ld), torch.float32)
    e = _fill(eps.region, c, 1)
    (a, av), (b, bv), (x, xv) = src(2), src(3, positive=True), src(4)
    for in_place in (False, True):
        tag = " in place" if in_place else ""
        out = guard.guarded((nvox, ld), dtype)
        # square (no alias allowed by its contract: out of place only)
        if not in_place:
            _lib.check(L.mri3d_bayes_square(P(x.region), P(out.region), nvox, c, ld, ld, dt, st), "square")
            check(out, xv * xv, "bayes_square")
            out = guard.guarded((nvox, ld), dtype)
            _lib.check(L.mri3d_bayes_sample_bwd(P(a.region), P(b.region), P(eps.region), P(out.region), nvox, c, ld, ld, ld, ld, dt, st), "sample_bwd")
            check(out, av * e / (2 * torch.sqrt(1e-4 + bv)), "bayes_sample_bwd")
            out = guard.guarded((nvox, ld), dtype)
        dst = out
        if in_place:
            dst, _ = src(2)          # a copy of `a` that the kernel overwrites
        _lib.check(L.mri3d_bayes_sample_fwd(P(dst.region if in_place else a.region), P(b.region), P(eps.region), P(dst.region), nvox, c,
                                            ld, ld, ld, ld, dt, st), "sample_fwd")
        check(dst, av + e * torch.sqrt(1e-4 + bv), "bayes_sample_fwd" + tag, in_place)
        dst = guard.guarded((nvox, ld), dtype)
        if in_place:
            dst, _ = src(2)
        _lib.check(L.mri3d_bayes_dx(P(dst.region if in_place else a.region), P(b.region), P(x.region), P(dst.region), nvox, c, ld, ld, ld,
                                    ld, dt, st), "dx")
        check(dst, av + 2 * xv * bv, "bayes_dx" + tag, in_place)
    for gd in (a, b, x, eps):       # inputs were only read
        gd.assert_guards_intact("input")


def test_weight_kernels_stay_inside_guard_bands():
    from mri_epilepsy_diagnosis_amd import _lib
    L = _lib.lib()
    ops = _ops()
    n = 1000                       # not a multiple of the block size
    mu, ls = draw_weights((n,), 7)
    mu_d, ls_d, up = mu.to(DEV), ls.to(DEV), torch.randn(3, n, device=DEV)
    st, P = ops._stream(), ops._ptr
    for evaluate in (0, 1):
        outs = [guard.guarded(n, torch.float32) for _ in range(5)]      # w_mean, w_var, log_alpha, dmu, dlogsigma
        _lib.check(L.mri3d_bayes_weights_fwd(P(mu_d), P(ls_d), n, evaluate, 3.0, P(outs[0].region), P(outs[1].region), P(outs[2].region), st), "fwd")
        _lib.check(L.mri3d_bayes_weights_bwd(P(mu_d), P(ls_d), n, evaluate, 3.0, P(up[0]), P(up[1]), P(up[2]), P(outs[3].region),
                                             P(outs[4].region), st), "bwd")
        torch.cuda.synchronize()
        for i, gd in enumerate(outs):
            gd.assert_guards_intact("weights output %d" % i)
            written = not gd.untouched().any()
            assert written == (i > 0 or evaluate == 1), (i, evaluate)   # train mode does not write w_mean
            if written:
                assert torch.isfinite(gd.region).all()


# ----------------------------------------------------------------------------------------------- operator, bf16
def _composed_bf16(case, t):
    """The same layer from what the project had before the fused kernels: ops.conv3d twice under autocast plus torch elementwise
    operations on the device (each of which rounds to bf16 once more)."""
    ops = _ops()
    n, ci, co, vol, k, stride, pad, bias, mode = case
    x = t["x"].to(DEV).to(BF).contiguous(memory_format=CL3D).requires_grad_(ci > 1)
    p = {key: (None if t[key] is None else t[key].to(DEV).requires_grad_()) for key in ("mu", "ls", "mb", "lb")}
    w_mean, w_var, la = bayes_ref.weight_transform(p["mu"], p["ls"], mode == "train", 3)
    with ops.autocast():
        mean = ops.conv3d(x, w_mean, p["mb"], stride, pad, 1)
        var = ops.conv3d(x * x, w_var, None if p["lb"] is None else p["lb"] ** 2, stride, pad, 1)
    y = (mean + (t["eps"].to(DEV) * torch.sqrt(1e-4 + var.float())).to(BF))
    ((y.float() * t["gy"].to(DEV)).sum() + (la * t["ga"].to(DEV)).sum()).backward()
    res = {"y": y.detach(), "log_alpha": la.detach(), "dx": x.grad, "dmu_weight": p["mu"].grad, "dlogsigma_weight": p["ls"].grad}
    if bias:
        res.update(dmu_bias=p["mb"].grad, dlogsigma_bias=p["lb"].grad)
    return res


@pytest.mark.parametrize("idx", [0, 2], ids=[IDS[0], IDS[2]])
def test_bayes_conv3d_bf16(idx):
    """Under ops.autocast(), inputs rounded to bf16 first.  Per tensor: within test_bf16_gpu._close's bar of the float64
    restatement, or no more than 1.5x as far from it as the composition of existing operators (the fused kernels round once where
    the composition rounds three times, so they should not be worse)."""
    from test_bf16_gpu import _close
    case = CASES[idx]
    t = dict(_case_tensors(case))
    t["x"], t["gy"] = t["x"].to(BF).float(), t["gy"].to(BF).float()
    ref = _reference(case, t)
    got = _product(case, t, cast=True)
    assert got["y"].dtype == BF and got["dx"].dtype == torch.float32 and got["dmu_weight"].dtype == torch.float32
    comp = _composed_bf16(case, t)
    failures = []
    for name in ref:
        r = ref[name].float()
        g_, c_ = (to_ncdhw(v).float() if v.dim() == 5 else v.detach().float().cpu() for v in (got[name], comp[name]))
        e_fused, e_comp = (g_ - r).abs().max().item(), (c_ - r).abs().max().item()
        try:
            _close(g_, r, name)
            inside = True
        except AssertionError:
            inside = False
        print("bf16 %s %s: |fused - f64| %.3e  |composed - f64| %.3e  scale %.3e  inside _close: %s"
              % (IDS[idx], name, e_fused, e_comp, r.abs().max().item(), inside))
        if not (inside or e_fused <= 1.5 * e_comp):
            failures.append((name, e_fused, e_comp))
    assert not failures, failures


# ----------------------------------------------------------------------------------------------- model
CHANNELS = [1, 4, 8, 8, 16]


def _sq(o):
    return (o ** 2).mean()


def _record_noise(model, x, seed):
    tape = bayes_ref.NoiseTape(seed=seed).install(model)
    with torch.no_grad():
        model(x)
    return tape.recorded


@pytest.mark.parametrize("bayes,train", [(True, True), (True, False), (False, True)], ids=["bayes-train", "bayes-eval", "plain-train"])
def test_unet3d_matches_restatement_with_injected_noise(bayes, train):
    """The bars of test_models_gpu._compare: output and loss 1e-3; each parameter gradient within 3e-2 of float64, or 4x
    torch-CPU-fp32's own distance, or 1e-5 of the largest gradient.  _compare strict-loads the restatement's weights."""
    from mri_epilepsy_diagnosis_amd.segmentation.models.bayes_unet import UNet3D
    from test_models_gpu import _compare
    torch.manual_seed(11)
    orc = bayes_ref.UNet3D(2, CHANNELS, bayes=bayes, shorten=True)
    prod = UNet3D(2, CHANNELS, bayes=bayes, shorten=True)
    x = seeded_randn(12, (2, 1, 16, 16, 32))
    noise = _record_noise(orc, x, 13)
    assert len(noise) == (19 if bayes else 0)
    bayes_ref.NoiseTape(noise).install(orc)       # copied with the model for the float64 run
    bayes_ref.NoiseTape(noise).install(prod)
    _compare(prod, orc, x, _sq, _sq, train)
    if bayes:
        for layer in bayes_ref.bayes_layers(prod):
            assert layer.log_alpha is not None and layer.log_alpha.shape == layer.mu_weight.shape


@pytest.mark.parametrize("tag,bayes,train", [("bayes_train", True, True), ("bayes_eval", True, False), ("plain_train", False, True)])
def test_unet3d_matches_the_golden_record(tag, bayes, train):
    """The run recorded from the reference modules (tools/gen_bayes_golden.py): same seeded weights and input, the recorded noise."""
    from mri_epilepsy_diagnosis_amd.segmentation.models.bayes_unet import UNet3D
    from test_models_gpu import _compare
    gold = load_golden("bayes_unet.npz")
    torch.manual_seed(int(gold["model_seed"]))
    orc = bayes_ref.UNet3D(2, gold["channels"].tolist(), bayes=bayes, shorten=True)
    prod = UNet3D(2, gold["channels"].tolist(), bayes=bayes, shorten=True)
    noise = [torch.from_numpy(gold["noise_%02d" % i]) for i in range(19)]
    bayes_ref.NoiseTape(noise).install(orc)
    bayes_ref.NoiseTape(noise).install(prod)
    x = seeded_randn(int(gold["input_seed"]), tuple(gold["shape"]))
    rec = {k[len(tag) + 1:]: gold[k] for k in gold.files if k.startswith(tag + "_")}
    _compare(prod, orc, x, _sq, _sq, train, gold=rec)


# ----------------------------------------------------------------------------------------------- loop
def _two_batches(seed):
    from mri_epilepsy_diagnosis_amd import parallel
    from mri_epilepsy_diagnosis_amd.segmentation import routine
    from mri_epilepsy_diagnosis_amd.segmentation.models.bayes_unet import UNet3D
    torch.manual_seed(seed)
    model = UNet3D(2, CHANNELS, bayes=True, shorten=True).to(DEV)
    before = [p.detach().clone() for p in model.parameters()]
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    losses = routine.run_epoch(1, routine.Action.TRAIN, routine.synthetic_loader(2, 1, (16, 16, 32), DEV), model, opt)
    torch.cuda.synchronize()
    changed = [not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters())]
    cache = parallel.StepCache.of(model)
    return losses, changed, (cache.captures, cache.replays, cache.eager_runs)


def test_run_epoch_trains_the_bayes_unet_with_its_own_noise():
    losses, changed, stats = _two_batches(21)
    assert losses.shape == (2,) and np.isfinite(losses).all()
    assert all(changed)
    assert stats == (1, 2, 0), stats      # the step, noise included, was captured once and replayed for both batches
    again, _, _ = _two_batches(21)
    assert np.array_equal(losses, again), (losses, again)      # same seed: the same noise, the same losses, bit for bit
