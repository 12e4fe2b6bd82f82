"""CPU suite: the predicate, the workspace query and the route name of the first layer with its activation folded in
(mri3d_conv_cin1_act_*) are host decisions that agree with what the entry points do before any launch, and
`nn.fused_conv_act` leaves the two operators alone, with nothing run, where the predicate declines."""
import ctypes

import pytest
import torch

from mri_epilepsy_diagnosis_amd import _lib

FWD, BWD = _lib.PASS_FWD, _lib.PASS_WGRAD
CL = torch.channels_last_3d


def _geom(co=8, n=2, sp=(160, 192, 160), ci=1, k=3, s=1, p=1, d=1, x_ld=None, z_ld=None, dtype=_lib.F32):
    dd, hh, ww = sp
    out = tuple((e + 2 * p - d * (k - 1) - 1) // s + 1 for e in sp)
    return _lib.ConvGeom(n, dd, hh, ww, ci, *out, co, k, k, k, s, s, s, p, p, p, d, d, d, ci if x_ld is None else x_ld,
                         co if z_ld is None else z_ld, dtype)


def _route(g, a_ld, act, alpha_n, pass_, align=16):
    name = ctypes.create_string_buffer(64)
    assert _lib.lib().mri3d_conv_cin1_act_route(ctypes.byref(g), a_ld, act, alpha_n, pass_, align, name, 64) == 0, _lib.lib().mri3d_last_error()
    return name.value.decode()


def _launch(g, a_ld, act, alpha_n, pass_, ws_bytes, ptr=4096):
    """The entry point of the pass with made-up addresses: it returns before any launch unless the workspace suffices."""
    L = _lib.lib()
    fake, G = ctypes.c_void_p(ptr), ctypes.byref(g)
    if pass_ == FWD:
        return L.mri3d_conv_cin1_act_fwd(G, a_ld, act, alpha_n, 0.01, fake, fake, fake, fake, fake, fake, fake, ws_bytes, None)
    return L.mri3d_conv_cin1_act_bwd(G, a_ld, act, alpha_n, 0.01, fake, fake, fake, fake, fake, fake, fake, fake, ws_bytes, None)


SERVED = [dict(co=co, sp=sp, **kw) for co in (8, 16) for sp in ((160, 192, 160), (4, 8, 32), (5, 9, 33), (3, 3, 3), (1, 1, 1))
          for kw in (dict(), dict(x_ld=4), dict(x_ld=3, z_ld=co + 4), dict(z_ld=co + 8))]
ACTS = [(_lib.ACT_PRELU, 1), (_lib.ACT_PRELU, None), (_lib.ACT_LEAKY, 1), (_lib.ACT_RELU, 1)]      # None: one alpha per channel


@pytest.mark.parametrize("act,alpha_n", ACTS)
@pytest.mark.parametrize("kw", SERVED, ids=lambda kw: "_".join("%s%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in kw.items()))
def test_served_geometries_route_and_launch_agree(kw, act, alpha_n):
    L = _lib.lib()
    g, co = _geom(**kw), kw["co"]
    alpha_n = co if alpha_n is None else alpha_n
    for a_ld in (co, co + 4):
        for pass_, kind in ((FWD, "fwd"), (BWD, "bwd")):
            want = pass_ == FWD or co == 8       # sixteen channels: the plain weight gradient is an MFMA kernel, with its own sum order
            assert L.mri3d_conv_cin1_act_supported(ctypes.byref(g), a_ld, act, alpha_n, pass_, 16) == int(want)
            assert _route(g, a_ld, act, alpha_n, pass_) == ("cin1 act %s co%d" % (kind, co) if want else "none")
            need = L.mri3d_conv_cin1_act_workspace_bytes(ctypes.byref(g), pass_)
            assert need == (27 * co * 4 if pass_ == FWD else 256 * (28 * co * 4 + co * 8))
            # what the entry point does with it: past the predicate (and stopped by the workspace) exactly where the route has a name
            assert _launch(g, a_ld, act, alpha_n, pass_, need - 1) == (-4 if want else -2)
    if co == 8:   # the plain weight gradient of the layer is the kernel whose sum order the backward keeps
        from mri_epilepsy_diagnosis_amd import ops
        assert ops.conv_route(g, _lib.PASS_WGRAD) == "generic cin1 co8"


DECLINED = [
    dict(ci=2), dict(co=4), dict(co=12), dict(co=32), dict(co=1),                   # one input channel, 8 or 16 output channels
    dict(k=1, p=0), dict(k=5, p=2), dict(s=2), dict(p=0), dict(p=2, d=2),           # 3x3x3, stride 1, padding 1, dilation 1
    dict(dtype=_lib.BF16),                                                          # bf16 keeps the four launches
    dict(z_ld=10), dict(z_ld=9), dict(a_ld=10), dict(a_ld=4),                       # pitches: multiples of 4, at least Co
    dict(act=_lib.ACT_NONE), dict(act=9), dict(alpha_n=3), dict(alpha_n=0),
    dict(align=8), dict(align=4),
    dict(co=16, n=1024, sp=(1024, 1024, 1024)),                                     # 2^31 tiles
]


@pytest.mark.parametrize("kw", DECLINED, ids=lambda kw: "_".join("%s%s" % (k, v) for k, v in kw.items() if k != "sp"))
def test_declined_geometries(kw):
    L = _lib.lib()
    kw = dict(kw)
    act, alpha_n, align = kw.pop("act", _lib.ACT_PRELU), kw.pop("alpha_n", 1), kw.pop("align", 16)
    g = _geom(**{k: v for k, v in kw.items() if k != "a_ld"})
    a_ld = kw.get("a_ld", g.co)
    for pass_ in (FWD, BWD):
        assert L.mri3d_conv_cin1_act_supported(ctypes.byref(g), a_ld, act, alpha_n, pass_, align) == 0
        rc = _launch(g, a_ld, act, alpha_n, pass_, 1 << 30, ptr=4096 + (0 if align == 16 else align))
        assert rc in (-1, -2) and len(L.mri3d_last_error()) > 0       # refused on the host: an inconsistent geometry, or not served
        name = ctypes.create_string_buffer(64)
        rc = L.mri3d_conv_cin1_act_route(ctypes.byref(g), a_ld, act, alpha_n, pass_, align, name, 64)
        assert rc == -1 or (rc == 0 and name.value == b"none")


def test_argument_validation_without_a_device():
    L = _lib.lib()
    g = _geom()
    G, fake = ctypes.byref(g), ctypes.c_void_p(4096)
    assert L.mri3d_conv_cin1_act_supported(None, 8, _lib.ACT_PRELU, 1, FWD, 16) == 0
    assert L.mri3d_conv_cin1_act_supported(G, 8, _lib.ACT_PRELU, 1, _lib.PASS_DGRAD, 16) == 0       # there is no data gradient
    assert L.mri3d_conv_cin1_act_workspace_bytes(None, FWD) == 0 and L.mri3d_conv_cin1_act_workspace_bytes(G, _lib.PASS_DGRAD) == 0
    fwd, bwd = L.mri3d_conv_cin1_act_fwd, L.mri3d_conv_cin1_act_bwd
    assert fwd(G, 8, _lib.ACT_PRELU, 1, 0.0, None, fake, fake, fake, fake, fake, fake, 1 << 20, None) == -1        # x
    assert b"null pointer" in L.mri3d_last_error()
    assert fwd(G, 8, _lib.ACT_PRELU, 1, 0.0, fake, fake, fake, None, fake, fake, fake, 1 << 20, None) == -1        # PReLU, no alpha
    assert fwd(G, 8, _lib.ACT_RELU, 1, 0.0, fake, fake, None, None, fake, fake, None, 1 << 20, None) == -4         # no workspace
    assert fwd(G, 8, _lib.ACT_RELU, 1, 0.0, fake, fake, None, None, ctypes.c_void_p(4104), fake, fake, 1 << 20, None) == -2   # z at 8 bytes
    assert bwd(G, 8, _lib.ACT_PRELU, 1, 0.0, fake, None, fake, fake, fake, fake, fake, fake, 1 << 20, None) == -1  # z
    assert bwd(G, 8, _lib.ACT_PRELU, 1, 0.0, fake, fake, fake, fake, None, fake, fake, fake, 1 << 20, None) == -1  # dW
    assert bwd(G, 8, _lib.ACT_PRELU, 1, 0.0, fake, fake, ctypes.c_void_p(4100), fake, fake, None, None, fake, 1 << 20, None) == -2   # da at 4 bytes
    name = ctypes.create_string_buffer(64)
    assert L.mri3d_conv_cin1_act_route(G, 8, _lib.ACT_PRELU, 1, FWD, 16, name, 8) == -1                          # name buffer
    assert L.mri3d_conv_cin1_act_route(G, 8, _lib.ACT_PRELU, 1, _lib.PASS_DGRAD, 16, name, 64) == -1


def test_ops_predicate_answers_for_host_tensors():
    from mri_epilepsy_diagnosis_amd import ops
    x = torch.zeros(2, 1, 5, 9, 33)
    w8, w16, alpha = torch.zeros(8, 1, 3, 3, 3), torch.zeros(16, 1, 3, 3, 3), torch.full((1,), 0.25)
    assert ops.conv3d_act_supported(x, w8, "prelu", alpha) and ops.conv3d_act_supported(x, w16, "prelu", torch.zeros(16))
    assert ops.conv3d_act_supported(x, w8, "relu") and ops.conv3d_act_supported(x, w8, "leaky_relu")
    wide = torch.zeros(2, 4, 5, 9, 33).contiguous(memory_format=CL)
    assert ops.conv3d_act_supported(wide[:, 2:3], w8, "prelu", alpha)                    # x with a pitch of 4
    assert not ops.conv3d_act_supported(x, w8, "prelu", None)                             # PReLU without its alpha never runs
    assert not ops.conv3d_act_supported(x, w8, "prelu", torch.zeros(3))
    assert not ops.conv3d_act_supported(x, w8, None) and not ops.conv3d_act_supported(x, w8, "none")
    assert not ops.conv3d_act_supported(x.bfloat16(), w8, "prelu", alpha) and not ops.conv3d_act_supported(x.double(), w8, "prelu", alpha)
    assert not ops.conv3d_act_supported(x.clone().requires_grad_(True), w8, "prelu", alpha)   # there is no data gradient
    assert not ops.conv3d_act_supported(x, torch.zeros(4, 1, 3, 3, 3), "prelu", alpha)
    assert not ops.conv3d_act_supported(x, torch.zeros(8, 1, 1, 1, 1), "prelu", alpha)
    assert not ops.conv3d_act_supported(torch.zeros(2, 2, 5, 9, 33), torch.zeros(8, 2, 3, 3, 3), "prelu", alpha)
    with ops.autocast():
        assert not ops.conv3d_act_supported(x, w8, "prelu", alpha)                        # the convolution would store bf16
    with pytest.raises(RuntimeError, match="not served"):
        ops.conv3d_act(x.bfloat16(), w8, None, alpha, "prelu", 0.0)


def test_block_keeps_the_two_operators_where_the_predicate_declines(monkeypatch):
    """`nn.fused_conv_act` returns None, with nothing run, for every layer the fold does not serve; and hands a served one on."""
    from mri_epilepsy_diagnosis_amd import nn as mnn, ops
    calls = []
    monkeypatch.setattr(ops, "conv3d_act", lambda *a, **k: calls.append(a) or "ran")
    monkeypatch.setattr(ops, "conv3d", lambda *a, **k: pytest.fail("a declined layer ran something"))
    monkeypatch.setattr(ops, "norm_act", lambda *a, **k: pytest.fail("a declined layer ran something"))
    x = torch.zeros(1, 1, 4, 8, 32)
    act = mnn.PReLU()
    declined = [(mnn.Conv3d(1, 8, 3, padding=1), None, x), (mnn.Conv3d(1, 8, 3, padding=1), act, x.bfloat16()),
                (mnn.Conv3d(1, 8, 3, padding=1), act, x.clone().requires_grad_(True)), (mnn.Conv3d(1, 8, 3, padding=0), act, x),
                (mnn.Conv3d(1, 8, 3, padding=1, stride=2), act, x), (mnn.Conv3d(1, 8, 3, padding=2, dilation=2), act, x),
                (mnn.Conv3d(1, 4, 3, padding=1), act, x), (mnn.Conv3d(1, 8, 1), act, x),
                (mnn.Conv3d(2, 8, 3, padding=1), act, torch.zeros(1, 2, 4, 8, 32)), (mnn.Conv3d(1, 8, 3, padding=1), mnn.PReLU(3), x)]
    for conv, a, xin in declined:
        assert mnn.fused_conv_act(conv, a, xin) is None
    with ops.autocast():
        assert mnn.fused_conv_act(mnn.Conv3d(1, 8, 3, padding=1), act, x) is None
    assert calls == []
    conv = mnn.Conv3d(1, 8, 3, padding=1)
    assert mnn.fused_conv_act(conv, act, x) == "ran" and len(calls) == 1
    assert calls[0][1] is conv.weight and calls[0][2] is conv.bias and calls[0][3] is act.weight and calls[0][4] == "prelu"
    # the block's switch: off, the layer goes to the two operators (which on the host have nothing to run on)
    monkeypatch.setattr(ops, "conv3d", lambda *a, **k: "two operators")
    monkeypatch.setattr(mnn, "fused_norm_act", lambda norm, a, y, out=None: y)
    assert mnn.conv_norm_act(conv, None, act, x, fused_first=False) == "two operators" and len(calls) == 1
    assert mnn.conv_norm_act(conv, None, act, x) == "ran" and len(calls) == 2
