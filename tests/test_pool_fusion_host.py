"""CPU suite: the predicate and the workspace query of the fused norm + activation + MaxPool3d(2) are host decisions, the entry
points validate their arguments before any launch, and `ops.norm_act_pool_supported` answers for host tensors."""
import ctypes

import pytest
import torch

from mri_epilepsy_diagnosis_amd import _lib


def _geoms(c=16, n=2, sp=(160, 192, 160), dtype=_lib.F32, k=2, s=2, p=0, x_ld=None, s_ld=None, p_ld=None, instance=0, group_c=0,
           act=_lib.ACT_PRELU, alpha_n=1, out=None, pool_in_ld=None):
    d, h, w = sp
    s_ld = c if s_ld is None else s_ld
    g = _lib.NormGeom(n, d * h * w, c, c if x_ld is None else x_ld, s_ld, instance, act, alpha_n, 0.0, 1e-5, group_c, dtype)
    do, ho, wo = out if out is not None else tuple((e + 2 * p - k) // s + 1 for e in sp)
    pg = _lib.PoolGeom(n, d, h, w, do, ho, wo, c, k, k, k, s, s, s, p, p, p, s_ld if pool_in_ld is None else pool_in_ld,
                       c if p_ld is None else p_ld, dtype)
    return g, pg


def _ask(g, pg):
    L = _lib.lib()
    return (L.mri3d_norm_act_pool_supported(ctypes.byref(g), ctypes.byref(pg)),
            L.mri3d_norm_act_pool_workspace_bytes(ctypes.byref(g), ctypes.byref(pg)))


@pytest.mark.parametrize("c", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16])
def test_served_geometries(c, dtype):
    ok, need = _ask(*_geoms(c=c, dtype=dtype, sp=(80, 96, 80)))
    # per block 3 norm sums per channel in double, at most 1024 blocks; plus the combined sums
    assert ok == 1 and 0 < need <= 1024 * 8 * 3 * c + 8 * 3 * c
    ok, need = _ask(*_geoms(c=c, dtype=dtype, n=1, sp=(2, 2, 2)))       # one block
    assert ok == 1 and need == 8 * 3 * c + (12 * c + 7) // 8 * 8
    # pitched x, skip and pooled: multiples of 4 elements
    assert _ask(*_geoms(c=c, dtype=dtype, sp=(4, 6, 2), x_ld=c + 4, s_ld=c + 8, p_ld=c + 12))[0] == 1


@pytest.mark.parametrize("kw", [
    dict(sp=(8, 7, 8)), dict(sp=(7, 8, 8)), dict(sp=(8, 8, 9)),                     # odd extents
    dict(k=3), dict(k=3, p=1), dict(s=1), dict(k=2, s=2, p=1, out=(5, 5, 5)),       # not kernel 2 / stride 2 / padding 0
    dict(c=12), dict(c=6), dict(c=128), dict(c=2),                                  # c/4 not a power of two <= 16
    dict(instance=1), dict(instance=1, group_c=4),                                  # instance / group statistics
    dict(x_ld=18), dict(s_ld=18), dict(p_ld=18), dict(x_ld=12),                     # pitches: multiples of 4, at least c
    dict(pool_in_ld=20),                                                            # the pool's input is the skip tensor
    dict(dtype=7), dict(alpha_n=3), dict(act=9),
    dict(n=1, sp=(1024, 1024, 256)),                                                # one sample of 2^28 voxels x 16: not below 2^31
    dict(c=4, n=16, sp=(512, 512, 512)),                                            # n * vox = 2^31
    dict(out=(80, 96, 79)),                                                         # pooled extents that are not half the input's
])
def test_declined_geometries(kw):
    L = _lib.lib()
    g, pg = _geoms(**kw)
    assert _ask(g, pg) == (0, 0)
    # the entry points refuse on the host, before any launch
    fake = ctypes.c_void_p(4096)
    assert L.mri3d_norm_act_pool_fwd(ctypes.byref(g), ctypes.byref(pg), fake, None, None, None, None, fake, fake, fake, fake, None) == -2
    assert len(L.mri3d_last_error()) > 0
    assert L.mri3d_norm_act_pool_bwd(ctypes.byref(g), ctypes.byref(pg), 0, fake, fake, fake, fake, None, None, None, None, fake, fake,
                                     None, None, None, fake, 1 << 30, None) == -2


def test_sizes_just_below_the_limits_are_served():
    assert _ask(*_geoms(c=4, n=1, sp=(1024, 1024, 510)))[0] == 1       # 2^29 * 510/512 voxels x 4 channels < 2^31 elements
    assert _ask(*_geoms(c=4, n=1, sp=(1024, 1024, 512)))[0] == 0
    assert _ask(*_geoms(c=4, n=15, sp=(512, 512, 512)))[0] == 1        # 15 * 2^27 voxels < 2^31


def test_argument_validation_without_a_device():
    L = _lib.lib()
    g, pg = _geoms()
    G, PG = ctypes.byref(g), ctypes.byref(pg)
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    assert L.mri3d_norm_act_pool_supported(None, PG) == 0 and L.mri3d_norm_act_pool_supported(G, None) == 0
    assert L.mri3d_norm_act_pool_workspace_bytes(None, PG) == 0 and L.mri3d_norm_act_pool_workspace_bytes(G, None) == 0
    fwd = L.mri3d_norm_act_pool_fwd
    assert fwd(None, PG, fake, None, None, None, None, fake, fake, fake, fake, None) == -1
    assert fwd(G, None, fake, None, None, None, None, fake, fake, fake, fake, None) == -1
    assert fwd(G, PG, None, None, None, None, None, fake, fake, fake, fake, None) == -1         # x
    assert b"null pointer" in L.mri3d_last_error()
    assert fwd(G, PG, fake, None, None, None, None, fake, fake, fake, None, None) == -1         # index bytes
    assert fwd(G, PG, fake, fake, None, None, None, fake, fake, fake, fake, None) == -1         # mean only
    assert fwd(G, PG, fake, None, None, None, None, None, fake, fake, fake, None) == -1         # PReLU, no alpha
    assert fwd(G, PG, odd, None, None, None, None, fake, fake, fake, fake, None) == -1          # alignment of x
    assert fwd(G, PG, fake, None, None, None, None, fake, fake, fake, ctypes.c_void_p(4097), None) == -1   # ... of the index bytes
    need = L.mri3d_norm_act_pool_workspace_bytes(G, PG)
    bwd = L.mri3d_norm_act_pool_bwd
    tail = (None, None, None, None, fake, fake, None, None, None)      # mean, invstd, gamma, beta, alpha, dx, dgamma, dbeta, dalpha
    assert bwd(G, PG, 0, fake, fake, fake, fake, *tail, fake, need - 1, None) == -4             # workspace
    assert bwd(G, PG, 0, fake, fake, fake, fake, *tail, None, need, None) == -4
    assert bwd(G, PG, 1, fake, fake, fake, fake, *tail, fake, need, None) == -1                 # training needs statistics
    assert bwd(G, PG, 0, fake, None, fake, None, *tail, fake, need, None) == -1                 # dpool without index bytes
    assert bwd(G, PG, 0, fake, odd, fake, fake, *tail, fake, need, None) == -1                  # alignment of dskip
    assert bwd(G, PG, 0, None, fake, fake, fake, *tail, fake, need, None) == -1                 # x


def test_ops_predicate_answers_for_host_tensors():
    from mri_epilepsy_diagnosis_amd import ops
    CL = torch.channels_last_3d
    x = torch.zeros(1, 16, 4, 6, 2).contiguous(memory_format=CL)
    alpha = torch.full((1,), 0.25)
    assert ops.norm_act_pool_supported(x, 2, None, 0, "batch", "prelu", alpha)
    assert ops.norm_act_pool_supported(x.bfloat16(), 2, 2, 0, "running", "relu")
    assert ops.norm_act_pool_supported(x, 2, None, 0, "none", None)
    assert not ops.norm_act_pool_supported(x, 2, None, 0, "batch", "prelu", None)      # PReLU without its alpha never runs
    assert not ops.norm_act_pool_supported(x, 3, 2, 0, "batch", "prelu", alpha)
    assert not ops.norm_act_pool_supported(x, 2, None, 1, "batch", "prelu", alpha)
    for mode in ("instance", "group", "sync"):
        assert not ops.norm_act_pool_supported(x, 2, None, 0, mode, "prelu", alpha)
    assert not ops.norm_act_pool_supported(torch.zeros(1, 16, 4, 5, 2).contiguous(memory_format=CL), 2, None, 0, "batch", "prelu", alpha)
    assert not ops.norm_act_pool_supported(torch.zeros(1, 12, 4, 6, 2).contiguous(memory_format=CL), 2, None, 0, "batch", "prelu", alpha)
    assert not ops.norm_act_pool_supported(x.double(), 2, None, 0, "batch", "prelu", alpha)
    assert not ops.norm_act_pool_supported(torch.zeros(1, 16, 1, 1, 1), 2, None, 0, "batch", "prelu", alpha)   # nothing to pool
    # a channel slice of a wider NDHWC buffer: served when it starts on a 4-element boundary
    wide = torch.zeros(1, 24, 4, 6, 2).contiguous(memory_format=CL)
    assert ops.norm_act_pool_supported(wide[:, 4:20], 2, None, 0, "batch", "prelu", alpha)
    assert not ops.norm_act_pool_supported(wide[:, 2:18], 2, None, 0, "batch", "prelu", alpha)
