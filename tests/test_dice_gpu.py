"""GPU suite of the float-target softmax-Dice loss (csrc/loss.hip), the loss of every training step, and the recorded bits of both
target forms.

The loss is compared with oracle.losses.softmax_dice_loss in float64, fed the stored logits (tests/test_labels_gpu.py's convention):
  loss      relative error <= 1e-5
  gradient  absolute error <= 8 x max(e32, 2^-23 max|grad64|), e32 the distance of torch's CPU float32 autograd from float64 on that
            case (never taken from the device); bf16 storage adds 2^-8 |grad64| per element for the rounding of the stored gradient.

Launch plan (loss.hip: dice_fwd_blocks with the float form's cap kDiceMaxBlocks, dice_bwd_blocks): a block is 256 lanes; a sample gets
min(ceil(vox / 1024), 1024 / N) blocks in the forward and min(ceil(vox / 256), 2048, 4096 / N) in the backward.  5x7x9 = 315 voxels:
one block, a partial first trip.  7x11x37 = 2849 voxels: 3 blocks = 768 lanes in the forward, three whole trips and 545 voxels more;
12 blocks and one trip in the backward.  81x81x81 = 531 441 voxels: the backward's 2048 blocks = 524 288 lanes take one whole trip
and 7153 voxels more.  One kernel is instantiated per class count 2..8 and storage type; ct == 1 broadcasts one target channel."""
import ctypes
import json
import os

import pytest
import torch

import loss_cases
from guard import SentinelSlice, guarded
from loss_cases import BF, CL, F32, SMALL, TRIPS, logits_of, target_of
from mri_epilepsy_diagnosis_amd import _lib, ops
from oracle import losses

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
EVERY_C = [(2, 1), (2, 2), (3, 3), (4, 1), (5, 5), (6, 1), (7, 7), (8, 8)]
BITS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_family_bits.json")


def _grad_of(z, t, dtype):
    x = z.detach().to(dtype).clone().requires_grad_(True)
    loss = losses.softmax_dice_loss(x, t.to(dtype))
    loss.backward()
    return loss.detach(), x.grad.detach()


def _ref_parts(z, t):
    """float64 loss and gradient of the stored logits, and e32: how far torch's CPU float32 autograd is from that gradient."""
    l64, g64 = _grad_of(z, t, torch.float64)
    _, g32 = _grad_of(z, t, F32)
    return l64.item(), g64, (g32.double() - g64).abs().max().item()


def _bound(g64, e32, dtype):
    bound = torch.full_like(g64, 8.0 * max(e32, 2.0 ** -23 * g64.abs().max().item()))
    return bound + 2.0 ** -8 * g64.abs() if dtype == BF else bound


def _device_run(z, t):
    x = z.cuda().contiguous(memory_format=CL).requires_grad_(True)
    loss = ops.softmax_dice_loss(x, t.cuda().contiguous(memory_format=CL))
    loss.backward()
    return loss.detach(), x.grad


def _judge(what, loss, grad, l64, g64, e32, dtype):
    rel = abs(loss - l64) / abs(l64)
    err = (grad.cpu().double() - g64).abs()
    worst = (err / _bound(g64, e32, dtype)).max().item()
    print("%s: loss %.7f rel err %.2e; grad max err %.3e (max|grad| %.3e, e32 %.2e), worst err / bound %.3f"
          % (what, loss, rel, err.max().item(), g64.abs().max().item(), e32, worst))
    assert bool(torch.isfinite(grad.float()).all()), what
    assert rel <= 1e-5, "%s: loss %.8f vs %.8f" % (what, loss, l64)
    assert worst <= 1.0, "%s: gradient error is %.2f x its bound" % (what, worst)


def _check(what, z, t, parts=None):
    l64, g64, e32 = _ref_parts(z, t) if parts is None else parts
    loss, grad = _device_run(z, t)
    assert loss.dtype == F32 and loss.shape == () and grad.dtype == z.dtype and grad.shape == z.shape
    _judge(what, loss.item(), grad, l64, g64, e32, z.dtype)


# one case per instantiation dice_{fwd,bwd}_kernel<T, C>
@BOTH
@pytest.mark.parametrize("C,ct", EVERY_C)
def test_float_dice_against_float64(C, ct, dtype):
    _check("C=%d ct=%d %s" % (C, ct, dtype), logits_of(C, SMALL, dtype, 1400 + 10 * C + ct), target_of(ct, SMALL, 1500 + 10 * C + ct))


@BOTH
@pytest.mark.parametrize("C,ct", [(2, 1), (3, 3)])
def test_float_dice_beyond_the_first_trip(C, ct, dtype):
    _check("trips C=%d ct=%d %s" % (C, ct, dtype), logits_of(C, TRIPS, dtype, 1600 + C), target_of(ct, TRIPS, 1700 + C))


@pytest.fixture(scope="module")
def big_case():
    """81x81x81 logits holding bfloat16 values: the float32 and the bfloat16 case share one float64 reference."""
    z, t = logits_of(3, (81, 81, 81), BF, 1803), target_of(3, (81, 81, 81), 1903)
    return z, t, _ref_parts(z, t)


@BOTH
def test_float_dice_backward_beyond_the_first_trip(dtype, big_case):
    z, t, parts = big_case
    assert z[0, 0].numel() > 2048 * 256
    _check("backward trips %s" % dtype, z.to(dtype), t, parts)


@BOTH
def test_float_dice_soft_targets(dtype):
    t = target_of(3, SMALL, 2003, soft=True)
    assert 0.0 < t.min().item() < 0.01 and 0.99 < t.max().item() < 1.0 and int(((t > 0.25) & (t < 0.75)).sum()) > 300
    _check("soft %s" % dtype, logits_of(3, SMALL, dtype, 2000), t)


@BOTH
@pytest.mark.parametrize("C,ct,x_ld,t_ld", [(2, 1, 5, 3), (3, 3, 4, 5), (8, 8, 11, 8), (8, 1, 8, 1)])
def test_float_dice_pitched_operands_and_guard_bands(C, ct, x_ld, t_ld, dtype):
    """Logits, target and gradient as channel slices [0, C) / [0, ct) of wider NDHWC buffers through the raw entry points: the other
    channels hold huge logits and NaN targets that must not be read, and sentinels that must not be written; dlogits, stats and the
    loss sit between guard bands."""
    z, t = logits_of(C, SMALL, dtype, 1000 + 10 * C + ct), target_of(ct, SMALL, 1100 + 10 * C + ct)
    l64, g64, e32 = _ref_parts(z, t)
    wide = torch.full((2,) + SMALL + (x_ld,), 3.0e4, dtype=dtype, device="cuda")           # exp(3e4) would be inf
    wide[..., :C] = z.permute(0, 2, 3, 4, 1).cuda()
    tw = torch.full((2,) + SMALL + (t_ld,), float("nan"), dtype=F32, device="cuda")
    tw[..., :ct] = t.permute(0, 2, 3, 4, 1).cuda()
    dz = SentinelSlice(2, x_ld, SMALL, dtype, 0, C)
    stats, loss = guarded(2 * C * 3, F32), guarded(1, F32)
    L = _lib.lib()
    g = _lib.DiceGeom(2, t[0, 0].numel(), C, ct, x_ld, t_ld, 1e-9, _lib.BF16 if dtype == BF else _lib.F32)
    ws = torch.empty(L.mri3d_softmax_dice_workspace_bytes(ctypes.byref(g)), dtype=torch.uint8, device="cuda")
    dloss = torch.ones(1, device="cuda")
    rc = L.mri3d_softmax_dice_fwd(ctypes.byref(g), ops._ptr(wide), ops._ptr(tw), ops._ptr(loss.region), ops._ptr(stats.region), ops._ptr(ws),
                                  ws.numel(), ops._stream())
    assert rc == 0, L.mri3d_last_error()
    rc = L.mri3d_softmax_dice_bwd(ctypes.byref(g), ops._ptr(wide), ops._ptr(tw), ops._ptr(stats.region), ops._ptr(dloss), ops._ptr(dz.slice),
                                  ops._stream())
    assert rc == 0, L.mri3d_last_error()
    torch.cuda.synchronize()
    dz.assert_outside_intact("pitched dlogits")
    stats.assert_guards_intact("stats"), loss.assert_guards_intact("loss")
    assert not bool(dz.slice_untouched().any()) and not bool(stats.untouched().any())
    _judge("pitched C=%d ct=%d" % (C, ct), loss.region.item(), dz.slice, l64, g64, e32, dtype)
    # stats are (tp, sum_p, sum_g) per (n, c): sum_g of a {0, 1} target is its exact count (ct == 1: the same for every class)
    st = stats.region.cpu().reshape(2, C, 3)
    assert torch.equal(st[..., 2], t.sum((2, 3, 4)).expand(2, C))
    assert torch.allclose(st[..., 1].sum(1), torch.full((2,), float(t[0, 0].numel())), rtol=1e-5)     # probabilities sum to one per voxel


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


@BOTH
@pytest.mark.parametrize("C,ct", [(2, 1), (8, 8)])
def test_float_dice_same_bits_run_to_run(C, ct, dtype):
    z, t = logits_of(C, TRIPS, dtype, 1200 + C), target_of(ct, TRIPS, 1300 + C)
    l1, g1 = _device_run(z, t)
    l2, g2 = _device_run(z, t)
    assert torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(g1), _bits(g2))


def test_both_forms_keep_their_recorded_bits():
    """tests/golden/loss_family_bits.json (tools/record_loss_bits.py): loss bits and gradient digest of both Dice target forms, of CE / focal alone
    and fused with the class-map Dice, and of the boundary loss, as one toolchain compiled them.  A change of the sources that is meant to keep the arithmetic keeps every case."""
    with open(BITS_FILE) as f:
        want = json.load(f)["cases"]
    cases = loss_cases.bit_cases()
    assert sorted(want) == sorted(c[0] for c in cases)
    bad = []
    for name, form, z, t, kw in cases:
        got = loss_cases.device_bits(ops, form, z, t, **kw)
        if got != want[name]:
            bad.append((name, got, want[name]))
    assert not bad, bad
