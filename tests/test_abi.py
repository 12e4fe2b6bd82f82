"""CPU suite: the C-ABI library loads and exports exactly the symbols include/mri3d.h declares."""
import ctypes
import os
import re
import subprocess

from mri_epilepsy_diagnosis_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mri3d.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mri3d_[a-z0-9_]+)\s*\(", src)))


def test_library_is_built():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"


def test_header_symbols_are_exported_and_bound():
    names = _declared()
    assert len(names) >= 20
    h = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(h, n), "library does not export %s" % n
    assert sorted(_lib.SIGNATURES) == names, (set(names) ^ set(_lib.SIGNATURES))


def test_no_unexpected_public_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\bT (mri3d_[a-z0-9_]+)$", out, flags=re.M)))
    assert exported == _declared()


def test_version_and_error_string_without_gpu():
    L = _lib.lib()
    assert L.mri3d_version() >= 100
    # argument validation happens on the host before any launch: safe without a device
    g = _lib.ConvGeom()
    rc = L.mri3d_conv3d_fwd(ctypes.byref(g), None, None, None, None, None, 0, None)
    assert rc == -1 or rc == -2
    assert len(L.mri3d_last_error()) > 0


def test_struct_layouts_match_header(tmp_path):
    """Compile the public header with gcc and compare sizeof/offsetof with the ctypes mirrors."""
    structs = {"Mri3dConvGeom": _lib.ConvGeom, "Mri3dNormGeom": _lib.NormGeom, "Mri3dPoolGeom": _lib.PoolGeom,
               "Mri3dUpGeom": _lib.UpGeom, "Mri3dDiceGeom": _lib.DiceGeom, "Mri3dNormPlanInfo": _lib.NormPlanInfo,
               "Mri3dResamplePlanInfo": _lib.ResamplePlanInfo, "Mri3dMarchPlanInfo": _lib.MarchPlanInfo,
               "Mri3dConvMfmaPlanInfo": _lib.ConvMfmaPlanInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mri3d.h"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            cf = "dout" if f == "dout" else f
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, cf))
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(out[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(out["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)


def test_workspace_queries_are_host_only():
    L = _lib.lib()
    g = _lib.ConvGeom(2, 160, 192, 160, 48, 160, 192, 160, 16, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 48, 16, 0)
    for p in (0, 1, 2):
        assert L.mri3d_conv3d_workspace_bytes(ctypes.byref(g), p) > 0
    # the fused autoencoder operators (round 3): predicates and workspace sizes are host decisions too
    # Conv3d(8, 1, (3,1,1), padding (1,0,0)) over a 4x nearest upsampling of 40x48x40 -> the virtual fine input 160x192x160
    up = _lib.ConvGeom(4, 160, 192, 160, 8, 160, 192, 160, 1, 3, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 8, 1, 0)
    assert L.mri3d_upconv3d_supported(ctypes.byref(up), 4) == 1 and L.mri3d_upconv3d_workspace_bytes(ctypes.byref(up), 4) > 0
    assert L.mri3d_upconv3d_supported(ctypes.byref(up), 3) == 0 and L.mri3d_upconv3d_workspace_bytes(ctypes.byref(up), 3) == 0
    wide = _lib.ConvGeom(4, 40, 48, 40, 16, 40, 48, 40, 8, 3, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 16, 8, 0)
    assert L.mri3d_upconv3d_supported(ctypes.byref(wide), 4) == 0          # 16 -> 8: no instance, the caller keeps the two operators
    # Conv3d(1, 8, (6,1,1), s (2,1,1), p (2,0,0)) then Conv3d(8, 8, (1,6,1), s (1,2,1), p (0,2,0)) on 160x192x160
    first = _lib.ConvGeom(4, 160, 192, 160, 1, 80, 192, 160, 8, 6, 1, 1, 2, 1, 1, 2, 0, 0, 1, 1, 1, 1, 8, 0)
    second = _lib.ConvGeom(4, 80, 192, 160, 8, 80, 96, 160, 8, 1, 6, 1, 1, 2, 1, 0, 2, 0, 1, 1, 1, 8, 8, 0)
    assert L.mri3d_convpair_supported(ctypes.byref(first), ctypes.byref(second)) == 1
    assert L.mri3d_convpair_workspace_bytes(ctypes.byref(first), ctypes.byref(second)) > 0
    assert L.mri3d_convpair_supported(ctypes.byref(second), ctypes.byref(first)) == 0


def test_norm_plan_query_is_declared_bound_and_host_only():
    assert "mri3d_norm_plan_query" in _declared() and "mri3d_norm_plan_query" in _lib.SIGNATURES
    src = open(HEADER).read()
    for i, name in enumerate(("STATS", "FWD", "BWD")):
        assert re.search(r"MRI3D_NORM_PASS_%s\s*=\s*%d\b" % (name, i), src) and getattr(_lib, "NORM_PASS_" + name) == i
    L = _lib.lib()
    g = _lib.NormGeom(2, 160 * 192 * 160, 16, 16, 16, 0, _lib.ACT_PRELU, 1, 0.0, 1e-5, 0, _lib.BF16)
    info = _lib.NormPlanInfo()
    assert L.mri3d_norm_plan_query(ctypes.byref(g), _lib.NORM_PASS_FWD, 16, ctypes.byref(info)) == 0
    assert (info.vec, info.CL, info.VT, info.cy, info.nblk, info.groups, info.gvox) == (8, 2, 128, 1, 1024, 1, 2 * 160 * 192 * 160)
    assert L.mri3d_norm_plan_query(ctypes.byref(g), _lib.NORM_PASS_BWD, 16, ctypes.byref(info)) == 0 and info.vec == 4
    assert L.mri3d_norm_plan_query(ctypes.byref(g), 7, 16, ctypes.byref(info)) == -1
    assert L.mri3d_norm_plan_query(None, _lib.NORM_PASS_FWD, 16, ctypes.byref(info)) == -1
    assert L.mri3d_norm_plan_query(ctypes.byref(g), _lib.NORM_PASS_FWD, 16, None) == -1


def test_resample_plan_queries_are_declared_bound_and_host_only():
    for name in ("mri3d_maxpool3d_plan_query", "mri3d_upsample3d_plan_query"):
        assert name in _declared() and name in _lib.SIGNATURES
    assert [f for f, _ in _lib.ResamplePlanInfo._fields_] == ["vec", "npv", "hch", "grid", "segs", "segl", "tiles_h", "tiles_w", "passes",
                                                              "items", "tables", "lds_bytes"]
    L = _lib.lib()
    info = _lib.ResamplePlanInfo()
    # the 16-channel decoder level of a full-size volume: 2 x 80x96x80 coarse, 1200 items of 16 planes; 2400 items in the backward
    ug = _lib.UpGeom(2, 80, 96, 80, 160, 192, 160, 16, 16, 16, _lib.UP_TRILINEAR, 0, 0.5, 0.5, 0.5, _lib.F32)
    assert L.mri3d_upsample3d_plan_query(ctypes.byref(ug), _lib.PASS_FWD, 16, ctypes.byref(info)) == 0
    assert (info.vec, info.npv, info.segs, info.segl, info.tiles_h, info.tiles_w, info.passes, info.items, info.grid) == \
        (4, 4, 5, 16, 24, 5, 1, 1200, 1200)
    assert L.mri3d_upsample3d_plan_query(ctypes.byref(ug), _lib.PASS_DGRAD, 16, ctypes.byref(info)) == 0
    assert (info.vec, info.segs, info.tiles_h, info.tiles_w, info.passes, info.items, info.grid, info.tables) == (4, 10, 24, 5, 1, 2400, 2400, 0)
    assert L.mri3d_upsample3d_plan_query(ctypes.byref(ug), _lib.PASS_WGRAD, 16, ctypes.byref(info)) == -1
    assert L.mri3d_upsample3d_plan_query(None, _lib.PASS_FWD, 16, ctypes.byref(info)) == -1
    assert L.mri3d_upsample3d_plan_query(ctypes.byref(ug), _lib.PASS_FWD, 16, None) == -1
    pg = _lib.PoolGeom(2, 2, 26, 80, 1, 13, 40, 16, 2, 2, 2, 2, 2, 2, 0, 0, 0, 16, 16, _lib.F32)
    assert L.mri3d_maxpool3d_plan_query(ctypes.byref(pg), _lib.PASS_FWD, 0, 16, 16, ctypes.byref(info)) == 0
    assert (info.vec, info.hch, info.grid, info.items, info.lds_bytes) == (4, 6, 6, 0, 0)       # 2 planes x chunks of 6, 6 and 1 rows
    assert L.mri3d_maxpool3d_plan_query(ctypes.byref(pg), _lib.PASS_DGRAD, 16, 16, 16, ctypes.byref(info)) == 0 and info.hch == 6
    assert L.mri3d_maxpool3d_plan_query(ctypes.byref(pg), _lib.PASS_FWD, 16, 16, 16, ctypes.byref(info)) == -1    # an addend in the forward
    assert L.mri3d_maxpool3d_plan_query(None, _lib.PASS_FWD, 0, 16, 16, ctypes.byref(info)) == -1
    assert L.mri3d_maxpool3d_plan_query(ctypes.byref(pg), _lib.PASS_FWD, 0, 16, 16, None) == -1


def test_fusedconv_plan_queries_are_declared_bound_and_host_only(tmp_path):
    for name in ("mri3d_upconv3d_plan_query", "mri3d_convpair_plan_query"):
        assert name in _declared() and name in _lib.SIGNATURES
    fields = ["hch", "grid", "gtrips", "trips", "per", "passes", "chunks", "slabs", "rows"]
    assert [f for f, _ in _lib.FusedConvPlanInfo._fields_] == fields
    # the layout of the struct against the header, as test_struct_layouts_match_header does for the others
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mri3d.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(Mri3dFusedConvPlanInfo));']
    lines += ['printf("%s %%zu\\n", offsetof(Mri3dFusedConvPlanInfo, %s));' % (f, f) for f in fields] + ["return 0;}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_lib.FusedConvPlanInfo)
    for f in fields:
        assert int(out[f]) == getattr(_lib.FusedConvPlanInfo, f).offset, f
    L = _lib.lib()
    info = _lib.FusedConvPlanInfo()

    def nums(*names):
        return tuple(getattr(info, f) for f in names)
    # the shipped last UpBlock: Conv3d(8, 1, (3,1,1), padding (1,0,0)) over a 4x nearest upsampling of 4 x 40x48x40
    up = _lib.ConvGeom(4, 160, 192, 160, 8, 160, 192, 160, 1, 3, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 8, 1, 0)
    assert L.mri3d_upconv3d_plan_query(ctypes.byref(up), 4, _lib.PASS_FWD, ctypes.byref(info)) == 0
    assert nums(*fields) == (6, 4096, 5, 4, 0, 0, 0, 4 * 160 * 32, 0)           # slabs of 6 rows x 160: 960 voxels, 4 lane trips
    assert L.mri3d_upconv3d_plan_query(ctypes.byref(up), 4, _lib.PASS_WGRAD, ctypes.byref(info)) == 0
    assert nums(*fields) == (6, 1024, 20, 4, 0, 0, 0, 4 * 160 * 32, 0)
    assert L.mri3d_upconv3d_plan_query(ctypes.byref(up), 4, _lib.PASS_DGRAD, ctypes.byref(info)) == 0
    assert nums(*fields) == (0, 4 * 40 * 48, 1, 0, 4, 10, 0, 0, 4 * 40 * 48)
    up2 = _lib.ConvGeom(4, 80, 96, 80, 8, 80, 96, 80, 1, 3, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 8, 1, 0)       # scale 2: 32 coarse voxels a pass
    assert L.mri3d_upconv3d_plan_query(ctypes.byref(up2), 2, _lib.PASS_DGRAD, ctypes.byref(info)) == 0
    assert nums("grid", "gtrips", "per", "passes", "rows") == (7680, 1, 32, 2, 7680)
    long_w = _lib.ConvGeom(1, 4, 4, 1028, 4, 4, 4, 1028, 1, 3, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 4, 1, 0)     # wo > 1024: one row, 5 trips
    assert L.mri3d_upconv3d_plan_query(ctypes.byref(long_w), 4, _lib.PASS_FWD, ctypes.byref(info)) == 0
    assert nums("hch", "trips", "slabs", "grid") == (1, 5, 16, 16)
    assert L.mri3d_upconv3d_plan_query(ctypes.byref(up), 3, _lib.PASS_FWD, ctypes.byref(info)) == -2        # as the entry points
    assert L.mri3d_upconv3d_plan_query(ctypes.byref(up), 4, 3, ctypes.byref(info)) == -1
    assert L.mri3d_upconv3d_plan_query(None, 4, _lib.PASS_FWD, ctypes.byref(info)) == -1
    assert L.mri3d_upconv3d_plan_query(ctypes.byref(up), 4, _lib.PASS_FWD, None) == -1
    # the shipped first DownBlock on 4 x 160x192x160: 4 * 80 * 192 rows, four per workgroup trip, 3 chunks of W
    first = _lib.ConvGeom(4, 160, 192, 160, 1, 80, 192, 160, 8, 6, 1, 1, 2, 1, 1, 2, 0, 0, 1, 1, 1, 1, 8, 0)
    second = _lib.ConvGeom(4, 80, 192, 160, 8, 80, 96, 160, 8, 1, 6, 1, 1, 2, 1, 0, 2, 0, 1, 1, 1, 8, 8, 0)
    assert L.mri3d_convpair_plan_query(ctypes.byref(first), ctypes.byref(second), ctypes.byref(info)) == 0
    assert nums(*fields) == (0, 1024, 15, 0, 0, 0, 3, 0, 4 * 80 * 192)
    assert L.mri3d_convpair_plan_query(ctypes.byref(second), ctypes.byref(first), ctypes.byref(info)) == -2
    assert L.mri3d_convpair_plan_query(None, ctypes.byref(second), ctypes.byref(info)) == -1
    assert L.mri3d_convpair_plan_query(ctypes.byref(first), ctypes.byref(second), None) == -1


def test_march_plan_query_is_declared_bound_and_host_only():
    from mri_epilepsy_diagnosis_amd import ops
    assert "mri3d_conv3d_march_plan_query" in _declared() and "mri3d_conv3d_march_plan_query" in _lib.SIGNATURES
    fields = ["chunks", "blocks", "wgh", "wgw", "gch", "gcw", "nseg", "seglen", "nbuf", "grid", "whole_chunks", "dispatcher", "smem_bytes",
              "wp_bytes"]
    assert [f for f, _ in _lib.MarchPlanInfo._fields_] == fields == list(ops.MARCH_PLAN_FIELDS)      # (layout: test_struct_layouts_match_header)
    L = _lib.lib()
    info = _lib.MarchPlanInfo()
    # the U-Net's full-resolution 16 -> 16 layer in bf16: 24 x 10 columns in 6 x 5 workgroups of 4 x 2, 8 segments of 20 planes
    g = _lib.ConvGeom(1, 160, 192, 160, 16, 160, 192, 160, 16, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 16, 16, _lib.BF16)
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), _lib.PASS_FWD, 1, ctypes.byref(info)) == 0
    got = {f: getattr(info, f) for f in fields}
    assert got == dict(chunks=1, blocks=1, wgh=4, wgw=2, gch=6, gcw=5, nseg=8, seglen=20, nbuf=3, grid=240, whole_chunks=1, dispatcher=1,
                       smem_bytes=14336 + 8 * 3 * 5760 + 8 * 32 * 8 + 64, wp_bytes=3 * 4608), got
    assert got["grid"] == L.mri3d_conv3d_march_stats_blocks(ctypes.byref(g))
    assert ops.conv_march_plan(g, _lib.PASS_DGRAD) == dict(got, dispatcher=1)
    g.dtype = _lib.F32
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), _lib.PASS_DGRAD, 0, ctypes.byref(info)) == 0
    assert (info.chunks, info.nbuf, info.wp_bytes, info.dispatcher) == (2, 2, 2 * 3 * 4608, 1)
    g.ci = g.x_ld = 40                                                                     # five fp32 chunks: as the entry points
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), _lib.PASS_FWD, 0, ctypes.byref(info)) == -2
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), _lib.PASS_DGRAD, 1, ctypes.byref(info)) == -1
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), _lib.PASS_WGRAD, 0, ctypes.byref(info)) == -1
    assert L.mri3d_conv3d_march_plan_query(None, _lib.PASS_FWD, 0, ctypes.byref(info)) == -1
    assert L.mri3d_conv3d_march_plan_query(ctypes.byref(g), _lib.PASS_FWD, 0, None) == -1


def test_mfma_plan_query_is_declared_bound_and_host_only():
    from mri_epilepsy_diagnosis_amd import ops
    assert "mri3d_conv3d_mfma_plan_query" in _declared() and "mri3d_conv3d_mfma_plan_query" in _lib.SIGNATURES
    fields = ["kernel", "ck", "chunks", "partial_chunk", "nt", "ntt", "gy", "tile_d", "tile_h", "tile_w", "tiles_d", "tiles_h", "tiles_w", "ntiles",
              "units", "grid", "mode", "split", "wbn", "cit", "cob", "tg", "p", "ci8", "co8", "segl", "max_tasks", "min_tasks", "chain", "stats_blocks",
              "workspace_bytes"]
    assert [f for f, _ in _lib.ConvMfmaPlanInfo._fields_] == fields == list(ops.MFMA_PLAN_FIELDS)      # (layout: test_struct_layouts_match_header)
    src = open(HEADER).read()
    for value, name in ops.MFMA_KERNELS.items():
        assert re.search(r"MRI3D_MFMA_%s\s*=\s*%d\b" % (name.upper(), value), src), name
    L = _lib.lib()
    info = _lib.ConvMfmaPlanInfo()
    # the U-Net's 48 -> 16 decoder layer in fp32 at 2 x 160x192x160: 19200 tiles of 4 x 8 x 16 on the persistent grid of 512, six chunks
    g = _lib.ConvGeom(2, 160, 192, 160, 48, 160, 192, 160, 16, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 48, 16, _lib.F32)
    assert L.mri3d_conv3d_mfma_plan_query(ctypes.byref(g), _lib.PASS_FWD, 1, 1, 0, 0, 16, 16, ctypes.byref(info)) == 0
    got = {f: getattr(info, f) for f in fields}
    assert got == dict(kernel=1, ck=8, chunks=6, partial_chunk=0, nt=1, ntt=1, gy=1, tile_d=4, tile_h=8, tile_w=16, tiles_d=40, tiles_h=24, tiles_w=10,
                       ntiles=19200, units=19200, grid=512, mode=0, split=0, wbn=0, cit=0, cob=0, tg=0, p=0, ci8=0, co8=0, segl=0, max_tasks=38,
                       min_tasks=37, chain=0, stats_blocks=512, workspace_bytes=6 * 14 * 1024), got
    assert got["stats_blocks"] == L.mri3d_conv3d_fwd_stats_blocks(ctypes.byref(g))
    assert ops.conv_mfma_plan(g, _lib.PASS_FWD, stats=True) == dict(got, kernel="tiled")
    # its weight gradient: wgrad6, three ci-tiles of 170 workgroups (21 or 22 per XCD group) walking 290 to 305 of the 51200 tiles of 2 x 6 x 16: chains of 305 x 48 products
    assert L.mri3d_conv3d_mfma_plan_query(ctypes.byref(g), _lib.PASS_WGRAD, 0, 0, 0, 0, 16, 16, ctypes.byref(info)) == 0
    assert (info.kernel, info.cit, info.cob, info.tg, info.p, info.ntiles, info.max_tasks, info.min_tasks, info.chain, info.workspace_bytes) == \
        (9, 3, 1, 27, 170, 51200, 305, 290, 305 * 48, 170 * 3 * 28 * 1024)
    assert L.mri3d_conv3d_mfma_plan_query(ctypes.byref(g), _lib.PASS_FWD, 0, 0, 0, 0, 8, 16, ctypes.byref(info)) == -2      # a generic kernel's
    g.dtype = _lib.BF16                                                                                                  # the marching kernel's
    assert L.mri3d_conv3d_mfma_plan_query(ctypes.byref(g), _lib.PASS_FWD, 0, 0, 0, 0, 16, 16, ctypes.byref(info)) == -2
    assert L.mri3d_conv3d_mfma_plan_query(ctypes.byref(g), _lib.PASS_DGRAD, 1, 0, 0, 0, 16, 16, ctypes.byref(info)) == -1
    assert L.mri3d_conv3d_mfma_plan_query(ctypes.byref(g), 3, 0, 0, 0, 0, 16, 16, ctypes.byref(info)) == -1
    assert L.mri3d_conv3d_mfma_plan_query(None, _lib.PASS_FWD, 0, 0, 0, 0, 16, 16, ctypes.byref(info)) == -1
    assert L.mri3d_conv3d_mfma_plan_query(ctypes.byref(g), _lib.PASS_FWD, 0, 0, 0, 0, 16, 16, None) == -1


def test_host_code_is_clean_under_address_and_ub_sanitizers():
    """the library's HOST side (argument validation, plan / dispatch selection, workspace sizing, error strings)
    built with -fsanitize=address,undefined and driven without a GPU by tests/native/host_sanitizer_driver.cpp: > 100 000
    workspace queries over every conv geometry family plus the validation branches of every entry point.  (GPU ASan is not
    available on this pool; the device code is covered by the -m gpu parity suite.)"""
    from mri_epilepsy_diagnosis_amd import build as B
    exe = B.build_host_sanitizer(verbose=False)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    assert "ran clean" in res.stdout
