"""GPU suite of the cross-entropy / focal family (csrc/ce_loss.hip): ops.softmax_ce_index_loss, ops.softmax_dice_ce_index_loss, the
raw entry points, segmentation/losses.py and their use through routine.run_epoch.

Every row of tests/ce_cases.py runs against ce_ref in float64, fed the logits after rounding to the storage type
(tests/test_labels_gpu.py's convention):
  loss      relative error <= 1e-5 (absolute where the reference is exactly 0: nothing counts)
  gradient  absolute error <= 8 x max(e32, 2^-23 max|grad64|), e32 the distance of torch's CPU float32 autograd from float64 on that
            case (measured against the reference, never against the kernel); bf16 storage adds 2^-8 |grad64| per element.
The launch plan each row is there for is in its `corner` and is held to ops.ce_index_plan by tests/test_ce_plan.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ce_cases
import ce_ref
import labels_ref
from ce_cases import BF, F32, case_id, group
from guard import SentinelSlice, guarded, kernels_launched
from mri_epilepsy_diagnosis_amd import _lib, ops, parallel
from mri_epilepsy_diagnosis_amd.segmentation import labels as label_maps, losses, routine
from mri_epilepsy_diagnosis_amd.unet import UNet
from oracle import losses as oracle_losses, unet_recon
from util import REL_TOL, seeded_randn

pytestmark = pytest.mark.gpu

CL = torch.channels_last_3d


def _device_run(c, z, lab, w, label_shape=None):
    x = z.cuda().contiguous(memory_format=CL).requires_grad_(True)
    t = lab.cuda() if label_shape is None else lab.cuda().reshape(label_shape)
    wd = None if w is None else w.cuda()
    if c.dice_weight == 0.0 and c.ce_weight == 1.0:
        loss = ops.softmax_ce_index_loss(x, t, wd, c.gamma)
    else:
        loss = ops.softmax_dice_ce_index_loss(x, t, c.dice_weight, c.ce_weight, wd, c.gamma)
    loss.backward()
    return loss.detach(), x.grad


def _judge(what, loss, grad, ref, dtype):
    l64, g64, e32 = ref
    ok, lerr, worst, finite = ce_ref.inside(loss.item(), grad.cpu(), l64, g64, e32, dtype)
    print("%s: loss %.7f (float64 %.7f) err %.2e; grad max|g64| %.3e, e32 %.2e, worst err / bound %.3f"
          % (what, loss.item(), l64, lerr, g64.abs().max().item(), e32, worst))
    assert finite, "%s: a value is not finite" % what
    assert lerr <= ce_ref.LOSS_REL, "%s: loss %.8f vs %.8f" % (what, loss.item(), l64)
    assert worst <= 1.0, "%s: gradient error is %.2f x its bound" % (what, worst)


def _check(c, label_shape=None):
    z, lab, w = ce_cases.inputs_of(c)
    ref = ce_ref.reference(z, lab, w, c.gamma, c.dice_weight, c.ce_weight)
    loss, grad = _device_run(c, z, lab, w, label_shape)
    assert loss.dtype == F32 and loss.shape == () and grad.dtype == z.dtype and grad.shape == z.shape
    _judge(case_id(c), loss, grad, ref, c.dtype)
    return loss, grad, ref


@pytest.mark.parametrize("c", group("base"), ids=case_id)
def test_against_float64(c):
    _check(c)


@pytest.mark.parametrize("c", group("fwd_trips"), ids=case_id)
def test_beyond_the_first_forward_trip(c):
    _check(c, (2, 1) + c.spatial)


@pytest.mark.parametrize("c", group("kinds"), ids=case_id)
def test_label_patterns(c):
    loss, grad, (l64, g64, _) = _check(c)
    if c.kind == "all_ignored":
        # nothing counts: the CE term is 0 with a zero gradient (torch gives NaN), the compound is dice_weight * Dice
        z, lab, _ = ce_cases.inputs_of(c)
        if c.dice_weight == 0.0:
            assert loss.item() == 0.0 and bool((grad.float() == 0).all())
        else:
            dl, _ = labels_ref.dice_index_ref(z, lab)
            assert abs(loss.item() - c.dice_weight * dl.item()) <= 1e-5 * abs(c.dice_weight * dl.item())


@pytest.mark.parametrize("c", group("confident"), ids=case_id)
def test_confident_logits(c):
    """Logits of scale 32: pt rounds to 1 where the label wins and to 0 where it loses by more than 88."""
    z, lab, _ = ce_cases.inputs_of(c)
    pt = torch.softmax(z.float(), 1).gather(1, lab.long().clamp_max(c.C - 1)[:, None])[:, 0][lab < c.C]
    assert int((pt == 1).sum()) >= 1 and int((pt == 0).sum()) >= 1
    _check(c)


def test_all_ones_weights_give_the_bits_of_no_weights():
    for C, dtype in ((2, F32), (9, BF), (32, F32)):
        c = next(r for r in group("base") if r.C == C and r.dtype == dtype and r.dice_weight > 0)
        z, lab, _ = ce_cases.inputs_of(c)
        l0, g0 = _device_run(c, z, lab, None)
        l1, g1 = _device_run(c, z, lab, torch.ones(C))
        bits = torch.int16 if dtype == BF else torch.int32
        assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and torch.equal(g0.view(bits), g1.view(bits))


@pytest.fixture(scope="module")
def big_case():
    """The latest (C, logits, labels, weights, float64 parts) of the backward's trip cases: the logits hold bfloat16 values, so the
    float32 and the bfloat16 case of one C (run one after the other) share one float64 reference."""
    return {}


@pytest.mark.parametrize("c", group("bwd_trips"), ids=case_id)
def test_backward_beyond_the_first_trip(c, big_case):
    if big_case.get("C") != c.C:
        big_case.clear()
        z, lab, w = ce_cases.inputs_of(c, BF)
        big_case.update(C=c.C, z=z, lab=lab, w=w, ref=ce_ref.reference(z, lab, w, c.gamma, c.dice_weight, c.ce_weight))
    z, lab, w = big_case["z"].to(c.dtype), big_case["lab"], big_case["w"]
    vox = lab[0].numel()
    assert vox % 2 == 1 and (vox // 4 if c.C == 2 else vox) > 2048 * 256
    loss, grad = _device_run(c, z, lab, w)
    _judge(case_id(c), loss, grad, big_case["ref"], c.dtype)


def _abi_fwd_bwd(c, logits_buf, dlogits_buf, lab, w, stats, loss):
    """The two entry points on raw NDHWC buffers of pitch c.pitch."""
    L = _lib.lib()
    n, vox = lab.shape[0], lab[0].numel()
    g = _lib.CeIndexGeom(n, vox, c.C, c.pitch, 1e-9, _lib.BF16 if c.dtype == BF else _lib.F32, c.gamma, c.dice_weight, c.ce_weight)
    ws = torch.empty(L.mri3d_softmax_ce_index_workspace_bytes(ctypes.byref(g)), dtype=torch.uint8, device="cuda")
    dloss = torch.ones(1, device="cuda")
    st = ops._stream()
    rc = L.mri3d_softmax_ce_index_fwd(ctypes.byref(g), ops._ptr(logits_buf), ops._ptr(lab), ops._ptr(w), ops._ptr(loss), ops._ptr(stats),
                                      ops._ptr(ws), ws.numel(), st)
    assert rc == 0, L.mri3d_last_error()
    rc = L.mri3d_softmax_ce_index_bwd(ctypes.byref(g), ops._ptr(logits_buf), ops._ptr(lab), ops._ptr(w), ops._ptr(stats), ops._ptr(dloss),
                                      ops._ptr(dlogits_buf), st)
    assert rc == 0, L.mri3d_last_error()
    torch.cuda.synchronize()


def _instantiation(name, dtype):
    """(bucket, Dice part) of a kernel name <storage type, bucket, Dice part> as the profiler reports it: demangled for float; the
    bfloat16 names come mangled (...IDF16bLi8ELb1E...) or, from a demangler that does not know the type, without their numbers:
    None then, after a look that the name is a bfloat16 one."""
    import re
    m = re.search(r"<float, (\d+), (true|false)>", name)
    if m:
        assert dtype == F32, name
        return int(m.group(1)), int(m.group(2) == "true")
    assert dtype == BF and "<float," not in name, name
    m = re.search(r"IDF16bLi(\d+)ELb([01])E", name)
    return (int(m.group(1)), int(m.group(2))) if m else None


@pytest.mark.parametrize("c", group("pitched"), ids=case_id)
def test_pitched_logits_and_guard_bands(c):
    """Logits and their gradient as channel slices [0, C) of pitch-channel buffers: the other channels hold huge logits that must not
    be read, and sentinels that must not be written; dlogits, stats and loss sit between guard bands.  The kernels that ran are the
    instantiation the plan names."""
    z, lab, w = ce_cases.inputs_of(c)
    ref = ce_ref.reference(z, lab, w, c.gamma, c.dice_weight, c.ce_weight)
    C, ld = c.C, c.pitch
    wide = torch.full((2,) + c.spatial + (ld,), 3.0e4, dtype=c.dtype, device="cuda")           # NDHWC memory; exp(3e4) would be inf
    wide[..., :C] = z.permute(0, 2, 3, 4, 1).cuda()
    dz = SentinelSlice(2, ld, c.spatial, c.dtype, 0, C)
    stats, loss = guarded(4 + 2 * C * 3, F32), guarded(1, F32)
    wd = None if w is None else w.cuda()
    _, names = kernels_launched(lambda: _abi_fwd_bwd(c, wide, dz.slice, lab.cuda(), wd, stats.region, loss.region))
    dz.assert_outside_intact("pitched dlogits")
    stats.assert_guards_intact("stats"), loss.assert_guards_intact("loss")
    assert not bool(dz.slice_untouched().any())
    _judge(case_id(c), loss.region[0], dz.slice, ref, c.dtype)
    st = stats.region.cpu()
    assert not bool(stats.untouched()[:4].any()) and bool(stats.untouched()[4:].all()) == (c.dice_weight == 0.0)
    wy = (torch.ones(C) if w is None else w)[lab.long().clamp_max(C - 1)] * (lab < C)
    assert abs(st[1].item() * wy.double().sum().item() - 1.0) <= 1e-6                       # 1 / sum_w
    if c.dice_weight:
        want_g = torch.stack([(lab.reshape(2, -1) == k).sum(1) for k in range(C)], 1).float()
        assert torch.equal(st[4:].reshape(2, C, 3)[..., 2], want_g)                           # sum_g is the exact count of the class
    plan = ops.ce_index_plan(2, lab[0].numel(), C, c.dtype, x_ld=ld, dice_weight=c.dice_weight, ce_weight=c.ce_weight, gamma=c.gamma)
    assert (plan["bucket"], plan["mode"], plan["dice"]) == (c.corner["bucket"], c.corner["mode"], c.corner["dice"])
    ours = sorted(k for k in names if "ce_index_" in k)
    assert len(ours) == 3 and any("ce_index_finalize_kernel" in k for k in ours), names
    for which in ("ce_index_fwd_kernel", "ce_index_bwd_kernel"):
        k = next(k for k in ours if which in k)
        assert _instantiation(k, c.dtype) in ((plan["bucket"], plan["dice"]), None), (k, plan)
    assert not any("dice_index" in k or "dice_finalize" in k for k in names), names


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [2, 9, 32])
def test_same_bits_run_to_run(C, dtype):
    for c in (r for r in group("fwd_trips") + group("base") if r.C == C and r.dtype == dtype):
        z, lab, w = ce_cases.inputs_of(c)
        l1, g1 = _device_run(c, z, lab, w)
        l2, g2 = _device_run(c, z, lab, w)
        bits = torch.int16 if dtype == BF else torch.int32
        assert torch.equal(l1.view(torch.int32), l2.view(torch.int32)) and torch.equal(g1.view(bits), g2.view(bits)), case_id(c)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [2, 5, 32])
def test_compound_is_the_weighted_sum_of_the_two_device_losses(C, dtype):
    c = next(r for r in group("kinds") if r.C == C and r.kind == "ignored" and r.dice_weight > 0)
    z, lab, w = ce_cases.inputs_of(c, dtype)
    x, t, wd = z.cuda().contiguous(memory_format=CL), lab.cuda(), None if w is None else w.cuda()
    both = ops.softmax_dice_ce_index_loss(x, t, c.dice_weight, c.ce_weight, wd, c.gamma).item()
    parts = c.dice_weight * ops.softmax_dice_index_loss(x, t).item() + c.ce_weight * ops.softmax_ce_index_loss(x, t, wd, c.gamma).item()
    assert abs(both - parts) <= 1e-6 * abs(parts), (both, parts)
    xg = x.clone().requires_grad_(True)
    ops.softmax_dice_ce_index_loss(xg, t, c.dice_weight, c.ce_weight, wd, c.gamma).backward()
    l64, g64, e32 = ce_ref.reference(z, lab, w, c.gamma, c.dice_weight, c.ce_weight)
    assert ce_ref.inside(both, xg.grad.cpu(), l64, g64, e32, dtype)[0]


def test_gamma_zero_is_torch_cross_entropy_on_the_device():
    c = next(r for r in group("kinds") if r.C == 5 and r.kind == "ignored" and r.dice_weight == 0)
    z, lab, _ = ce_cases.inputs_of(c, F32)
    w = ce_cases.weights_of("random", 5, 3)
    t = lab.long().clone()
    t[t >= 5] = -100
    want = F.cross_entropy(z.double(), t, weight=w.double(), ignore_index=-100).item()
    got = ops.softmax_ce_index_loss(z.cuda().contiguous(memory_format=CL), lab.cuda(), w.cuda()).item()
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)


def test_refusals_raise_before_any_launch():
    lab = torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device="cuda")

    def z(C):
        return torch.zeros(1, C, 4, 4, 4, device="cuda").contiguous(memory_format=CL)
    bad = [("classes must be in", lambda: ops.softmax_ce_index_loss(z(1), lab)),
           ("classes must be in", lambda: ops.softmax_dice_ce_index_loss(z(33), lab)),
           ("gamma must be 0 or in", lambda: ops.softmax_ce_index_loss(z(3), lab, gamma=0.5)),
           ("gamma must be 0 or in", lambda: ops.softmax_dice_ce_index_loss(z(3), lab, gamma=-1.0)),
           ("weight must be a float32 tensor of 3 entries", lambda: ops.softmax_ce_index_loss(z(3), lab, torch.ones(4, device="cuda"))),
           ("weight must be a float32 tensor of 3 entries", lambda: ops.softmax_ce_index_loss(z(3), lab, torch.ones(3, device="cuda").double())),
           ("weight must be a float32 tensor of 3 entries", lambda: ops.softmax_ce_index_loss(z(3), lab, torch.ones(3))),
           ("weight must be a float32 tensor of 3 entries", lambda: ops.softmax_ce_index_loss(z(3), lab, [1.0, 1.0, 1.0])),
           ("labels must be a uint8 class map", lambda: ops.softmax_ce_index_loss(z(3), lab.long())),
           ("labels shape", lambda: ops.softmax_ce_index_loss(z(3), lab[:, :2])),
           ("ROCm device", lambda: ops.softmax_ce_index_loss(z(3).cpu(), lab)),
           ("not both zero", lambda: ops.softmax_dice_ce_index_loss(z(3), lab, 0.0, 0.0)),
           ("not negative", lambda: ops.softmax_dice_ce_index_loss(z(3), lab, -1.0, 1.0))]
    for match, fn in bad:
        def run():
            with pytest.raises(RuntimeError, match=match):
                fn()
        _, names = kernels_launched(run)
        assert not any("ce_index" in k for k in names), (match, names)


# ------------------------------------------------------------------------------------------------ model level
IDS = [17, 53, 1006, 2035]       # -> classes 1..4, background 0


def _parcellation_batches(count):
    out = []
    for i in range(count):
        g = torch.Generator().manual_seed(60 + i)
        pick = torch.randint(0, 6, (1, 1, 16, 16, 16), generator=g)            # 4 ids of the map, 2 ids outside it
        raw = torch.tensor(IDS + [4, 3000])[pick].to(torch.int16)
        out.append({routine.MRI: {routine.DATA: seeded_randn(50 + i, (1, 1, 16, 16, 16))}, routine.LABEL: {routine.DATA: raw}})
    return out


def test_class_weights_come_from_exact_device_counts():
    lab = ce_cases.class_map_of("absent", 5, ce_cases.SMALL, 77)
    lab[lab == 3] = 0                                                              # class 3 occurs nowhere
    counts = np.bincount(lab.reshape(-1).numpy(), minlength=5)[:5]
    for rule in losses.RULES:
        w = losses.class_weights(lab.cuda(), 5, rule)
        assert w.is_cuda and w.dtype == F32 and w.shape == (5,)
        assert np.array_equal(w.cpu().numpy(), losses.weights_from_counts(counts, rule)) and w[3].item() == 0.0


def test_dice_ce_training_through_run_epoch_is_captured_once():
    lm = label_maps.LabelMap.from_ids(IDS)
    batches = _parcellation_batches(2)
    torch.manual_seed(0)
    orc = unet_recon.UNetRecon(out_classes=5, out_channels_first_layer=8)
    model = UNet(in_channels=1, out_classes=5, dimensions=3, num_encoding_blocks=3, out_channels_first_layer=8, normalization="batch",
                 upsampling_type="linear", padding=True, activation="PReLU")
    model.load_state_dict(orc.state_dict())
    model.cuda()

    def prepare(batch, dev):
        return label_maps.prepare_batch_index(batch, dev, lm)
    all_classes = torch.cat([prepare(b, "cuda")[1] for b in batches])
    w = losses.class_weights(all_classes, 5, "inverse_sqrt")
    opt = torch.optim.AdamW(model.parameters())
    got = []
    for b in batches:            # a loss built anew with equal settings for every epoch must not force a second capture
        got += routine.run_epoch(1, routine.Action.TRAIN, [b], model, opt, loss_fn=losses.DiceCELoss(weight=w), prepare=prepare).tolist()
    cache = parallel.StepCache.of(model)
    assert (cache.captures, cache.eager_runs, cache.replays) == (1, 0, 2) and not cache.disabled
    # the oracle on the CPU: the reference's Dice on a float one-hot target plus torch's cross-entropy
    oopt = torch.optim.AdamW(orc.parameters())
    orc.train()
    want = []
    for b in batches:
        classes = torch.from_numpy(labels_ref.remap_ref(b[routine.LABEL][routine.DATA].numpy(), lm.lut, 0, 0))
        oopt.zero_grad()
        logits = orc(b[routine.MRI][routine.DATA])
        loss = oracle_losses.softmax_dice_loss(logits, labels_ref.one_hot(classes, 5, F32)) + \
            F.cross_entropy(logits, classes[:, 0].long(), weight=w.cpu())
        loss.backward()
        oopt.step()
        want.append(loss.item())
    print("Dice + CE trajectory", got, "oracle", want)
    np.testing.assert_allclose(got, want, rtol=REL_TOL)
