"""CPU suite of the Monte-Carlo predictive statistics: the C ABI of csrc/mc_stats.hip (symbols, the host-only state query, every
validation branch, all before any launch), the no-fallback errors of the Python layers, the unet.UNet(monte_carlo_dropout=p)
option, and the float64 reference the GPU suite compares with (tests/mc_ref.py)."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import mc_ref
from mri_epilepsy_diagnosis_amd import _lib, nn as mnn, ops
from mri_epilepsy_diagnosis_amd.unet import UNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mri3d_mc_state_bytes", "mri3d_mc_accumulate", "mri3d_mc_finalize")
EINVAL, ENOTSUP = -1, -2
P = ctypes.c_void_p
FAKE = 0x10000          # a non-NULL address: validation never dereferences, and it returns before any launch


def test_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mri3d.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), "%s is not declared in mri3d.h" % n
        assert re.search(r"\bT %s$" % n, nm, flags=re.M), "%s is not exported" % n
        assert n in _lib.SIGNATURES


def test_state_query_is_host_only():
    q = _lib.lib().mri3d_mc_state_bytes
    assert q(1080, 2) > 0
    assert q(1080, 2) >= 1080 * (2 * 2 + 1) * 4          # sum p, sum p^2 per class and one sum p log p, fp32
    for c in range(2, 32):
        assert q(1080, c) <= q(1080, c + 1)
    for nvox in (1, 2, 3, 4, 5, 315, 1079, 1080, 1 << 20, (1 << 31) + 5):
        assert 0 < q(nvox, 2) <= q(nvox + 1, 2) and q(nvox, 3) <= q(nvox + 1, 3)
    for nvox, c in ((0, 2), (-1, 2), (-(1 << 40), 2), (1080, 1), (1080, 0), (1080, -3), (1080, 33)):
        assert q(nvox, c) == 0, (nvox, c)


def _accumulate(logits=FAKE, nvox=1080, c=2, ld=2, dtype=_lib.F32, reps=1, rep_stride=1080, first=1, state=FAKE, state_bytes=None):
    L = _lib.lib()
    if state_bytes is None or state_bytes == "one short":
        state_bytes = L.mri3d_mc_state_bytes(nvox, c) - (state_bytes is not None)
    return L.mri3d_mc_accumulate(P(logits), nvox, c, ld, dtype, reps, rep_stride, first, P(state), state_bytes, None)


def _finalize(state=FAKE, state_bytes=None, nvox=1080, c=2, samples=4, outs=(FAKE, FAKE, FAKE, FAKE, FAKE)):
    L = _lib.lib()
    if state_bytes is None or state_bytes == "one short":
        state_bytes = L.mri3d_mc_state_bytes(nvox, c) - (state_bytes is not None)
    return L.mri3d_mc_finalize(P(state), state_bytes, nvox, c, samples, *(P(o) for o in outs), None)


ACCUMULATE_BRANCHES = [
    ("NULL logits", dict(logits=None), EINVAL),
    ("NULL state", dict(state=None), EINVAL),
    ("nvox = 0", dict(nvox=0, state_bytes=1 << 20), EINVAL),
    ("c = 1", dict(c=1, ld=1, state_bytes=1 << 20), ENOTSUP),
    ("c = 33", dict(c=33, ld=33, state_bytes=1 << 20), ENOTSUP),
    ("c = 0", dict(c=0, state_bytes=1 << 20), ENOTSUP),
    ("unknown dtype", dict(dtype=7), ENOTSUP),
    ("ld < c", dict(c=3, ld=2), EINVAL),
    ("reps = 0", dict(reps=0), EINVAL),
    ("overlapping draws", dict(reps=2, rep_stride=1079), EINVAL),
    ("state one byte short", dict(state_bytes="one short"), EINVAL),
    ("state_bytes = 0", dict(state_bytes=0), EINVAL),
]

FINALIZE_BRANCHES = [
    ("NULL state", dict(state=None), EINVAL),
    ("nvox = 0", dict(nvox=0, state_bytes=1 << 20), EINVAL),
    ("c = 1", dict(c=1, state_bytes=1 << 20), ENOTSUP),
    ("c = 33", dict(c=33, state_bytes=1 << 20), ENOTSUP),
    ("samples = 0", dict(samples=0), EINVAL),
    ("no output", dict(outs=(None,) * 5), EINVAL),
    ("state one byte short", dict(state_bytes="one short"), EINVAL),
]


@pytest.mark.parametrize("what,kw,code", ACCUMULATE_BRANCHES, ids=[b[0] for b in ACCUMULATE_BRANCHES])
def test_accumulate_validation(what, kw, code):
    assert _accumulate(**kw) == code, what
    msg = _lib.lib().mri3d_last_error()
    assert msg and b"mc_accumulate" in msg, msg


@pytest.mark.parametrize("what,kw,code", FINALIZE_BRANCHES, ids=[b[0] for b in FINALIZE_BRANCHES])
def test_finalize_validation(what, kw, code):
    assert _finalize(**kw) == code, what
    msg = _lib.lib().mri3d_last_error()
    assert msg and b"mc_finalize" in msg, msg


def test_cpu_tensors_have_no_fallback():
    from mri_epilepsy_diagnosis_amd.segmentation import uncertainty
    logits = torch.zeros(1, 2, 4, 4, 4)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        ops.mc_accumulate(torch.zeros(1024), logits, True)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        ops.mc_state(logits.shape, "cpu")
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        ops.mc_finalize(torch.zeros(1024), logits.shape, 1)
    model = UNet(dimensions=3, padding=True, num_encoding_blocks=2, out_channels_first_layer=2, normalization="batch", monte_carlo_dropout=0.5)
    model.train()
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        uncertainty.mc_predict(model, torch.zeros(1, 1, 4, 4, 4), 2)
    assert all(m.training for m in model.modules())          # the modes come back also when the call raises


def test_unet_monte_carlo_dropout_option():
    kw = dict(in_channels=1, out_classes=2, dimensions=3, num_encoding_blocks=3, out_channels_first_layer=4, normalization="batch",
              upsampling_type="linear", padding=True, activation="PReLU")
    plain, mc = UNet(**kw), UNet(monte_carlo_dropout=0.5, **kw)
    assert list(mc.state_dict()) == list(plain.state_dict())
    assert plain.monte_carlo_layer is None
    assert isinstance(mc.monte_carlo_layer, mnn.Dropout3d) and isinstance(mc.monte_carlo_layer, torch.nn.Dropout3d)
    assert mc.monte_carlo_layer.p == 0.5
    UNet(dimensions=3, padding=True, monte_carlo_dropout=0.5)
    for bad in (dict(residual=True), dict(preactivation=True), dict(dropout=0.3), dict(padding_mode="reflect")):
        with pytest.raises(NotImplementedError):
            UNet(dimensions=3, padding=True, **bad)


def test_reference_agrees_with_a_direct_formulation():
    g = torch.Generator().manual_seed(0)
    for T, nvox, C in ((5, 200, 2), (3, 64, 3), (4, 50, 32)):
        z = (3.0 * torch.randn(T, nvox, C, generator=g)).double()
        r = mc_ref.mc_ref(z)
        p = torch.softmax(z, dim=2)
        mean = p.mean(0)
        ent = -(mean * mean.log()).sum(1)
        exp_ent = -(p * p.log()).sum(2).mean(0)
        assert (r["mean"] - mean).abs().max() < 1e-14
        assert (r["variance"] - p.var(0, unbiased=False)).abs().max() < 1e-14
        assert (r["entropy"] - ent).abs().max() < 1e-13
        assert (r["mutual_info"] - (ent - exp_ent)).abs().max() < 1e-13
        assert torch.equal(r["mask"].long(), mean.argmax(1))
        assert (r["sum_p2"] - (p * p).sum(0)).abs().max() < 1e-13 and (r["sum_plogp"] + T * exp_ent).abs().max() < 1e-12
        r32 = mc_ref.mc_ref(z, torch.float32)
        assert r32["mean"].dtype == torch.float32 and (r32["entropy"].double() - r["entropy"]).abs().max() < 1e-5


def test_reference_underflowed_class_contributes_exactly_zero():
    for dtype in (torch.float32, torch.float64):
        gap = 200.0 if dtype == torch.float32 else 2000.0      # exp(-gap) underflows to 0 in that precision
        r = mc_ref.mc_ref(torch.tensor([[[gap, 0.0], [0.0, gap]]]), dtype)
        assert r["sum_plogp"].tolist() == [0.0, 0.0]
        assert r["entropy"].tolist() == [0.0, 0.0] and r["mutual_info"].tolist() == [0.0, 0.0]
        assert r["mean"].tolist() == [[1.0, 0.0], [0.0, 1.0]] and r["mask"].tolist() == [0, 1]
        assert all(math.isfinite(v) for k in ("variance", "sum_p2") for v in r[k].flatten().tolist())
