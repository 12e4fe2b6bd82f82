"""CPU suite: the predicate and the workspace query of the fused norm + activation + pointwise head are host decisions, and the
entry points validate their arguments before any launch."""
import ctypes

import pytest

from mri_epilepsy_diagnosis_amd import _lib


def _geom(c, co, instance=0, x_ld=None, act=_lib.ACT_PRELU, alpha_n=1, dtype=_lib.F32, group_c=0, n=2, vox=160 * 192 * 160):
    return _lib.NormGeom(n, vox, c, c if x_ld is None else x_ld, co, instance, act, alpha_n, 0.0, 1e-5, group_c, dtype)


@pytest.mark.parametrize("c,co", [(4, 1), (8, 1), (16, 2), (32, 3), (64, 4)])
@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16])
def test_served_geometries(c, co, dtype):
    L = _lib.lib()
    g = _geom(c, co, dtype=dtype)
    assert L.mri3d_norm_act_pw_supported(ctypes.byref(g), co) == 1
    need = L.mri3d_norm_act_pw_workspace_bytes(ctypes.byref(g), co)
    # per block: 3 norm sums per channel and co * (c + 1) head sums, in double; at most 1024 blocks; plus the combined sums
    assert 0 < need <= 1024 * 8 * (3 * c + co * (c + 1)) + 8 * 3 * c
    small = _geom(c, co, dtype=dtype, n=1, vox=7)          # one block
    assert L.mri3d_norm_act_pw_workspace_bytes(ctypes.byref(small), co) == 8 * (3 * c + co * (c + 1)) + (12 * c + 7) // 8 * 8


@pytest.mark.parametrize("kw,co", [(dict(c=12), 2), (dict(c=6), 2), (dict(c=128), 2), (dict(c=16), 5), (dict(c=16), 0),
                                   (dict(c=16, instance=1), 2), (dict(c=16, instance=1, group_c=4), 2), (dict(c=16, x_ld=18), 2),
                                   (dict(c=16, alpha_n=3), 2), (dict(c=16, dtype=7), 2)])
def test_declined_geometries(kw, co):
    L = _lib.lib()
    g = _geom(co=co, **kw)
    assert L.mri3d_norm_act_pw_supported(ctypes.byref(g), co) == 0
    assert L.mri3d_norm_act_pw_workspace_bytes(ctypes.byref(g), co) == 0
    # the entry points refuse on the host, before any launch
    fake = ctypes.c_void_p(4096)
    assert L.mri3d_norm_act_pw_fwd(ctypes.byref(g), co, fake, None, None, None, None, fake, fake, None, fake, None) == -2
    assert len(L.mri3d_last_error()) > 0


def test_argument_validation_without_a_device():
    L = _lib.lib()
    g = _geom(16, 2)
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    assert L.mri3d_norm_act_pw_supported(None, 2) == 0 and L.mri3d_norm_act_pw_workspace_bytes(None, 2) == 0
    assert L.mri3d_norm_act_pw_fwd(None, 2, fake, None, None, None, None, fake, fake, None, fake, None) == -1
    assert L.mri3d_norm_act_pw_fwd(ctypes.byref(g), 2, None, None, None, None, None, fake, fake, None, fake, None) == -1    # x
    assert b"null pointer" in L.mri3d_last_error()
    assert L.mri3d_norm_act_pw_fwd(ctypes.byref(g), 2, fake, fake, None, None, None, fake, fake, None, fake, None) == -1    # mean only
    assert L.mri3d_norm_act_pw_fwd(ctypes.byref(g), 2, fake, None, None, None, None, None, fake, None, fake, None) == -1    # PReLU, no alpha
    assert L.mri3d_norm_act_pw_fwd(ctypes.byref(g), 2, odd, None, None, None, None, fake, fake, None, fake, None) == -1     # alignment
    need = L.mri3d_norm_act_pw_workspace_bytes(ctypes.byref(g), 2)
    args = (fake, fake, None, None, None, None, fake, fake, fake, None, None, None, None, None)
    assert L.mri3d_norm_act_pw_bwd(ctypes.byref(g), 2, 0, *args, fake, need - 1, None) == -4                                # workspace
    assert L.mri3d_norm_act_pw_bwd(ctypes.byref(g), 2, 1, *args, fake, need, None) == -1            # training needs statistics


def test_ops_predicate_declines_prelu_without_alpha(monkeypatch):
    """`act="prelu"` with `alpha=None` could never run: the predicate says so for every c and co (it is asked before any kernel, so
    a host tensor that claims to be on the device is enough)."""
    import torch
    from mri_epilepsy_diagnosis_amd import ops
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    x = torch.zeros(1, 16, 4, 6, 2).contiguous(memory_format=torch.channels_last_3d)
    for co in (1, 2, 4, 16):        # co = 1: a weight of c elements, which used to stand in for a per-channel alpha
        w = torch.zeros(co, 16, 1, 1, 1)
        assert ops.norm_act_pointwise_supported(x, w, "batch", "prelu", torch.full((1,), 0.25)) == (co <= 4)
        assert not ops.norm_act_pointwise_supported(x, w, "batch", "prelu", None)
