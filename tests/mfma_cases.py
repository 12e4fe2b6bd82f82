"""Rows of the parity suite of the 3x3x3 MFMA convolution family (tests/test_mfma_parity_gpu.py; their meaning: tests/mfma_run.py):
Conv3d 3x3x3 / padding 1 forward (with fused statistics), data gradient and weight gradient through mri3d_conv3d_fwd / _fwd_stats /
_dgrad / _wgrad and the *_cat forms, on the kernels of csrc/conv_mfma.hip (tiled, tiled_n8, direct) and csrc/conv_mfma_wgrad.hip
(cin1, wgrad3, wgrad4, wgrad6, bf16, bf16t).

  id       what the row is there for
  ci, co   channels;  n  batch;  sp  input extents (D, H, W);  stride  1, 2 or 3 (all axes)
  layout   {"x" | "y" | "x2": (channels of the wider buffer, first channel of the slice)}: x also places dx, y also places dy,
           x2 places the second tensor of a split operand (x2 forward and weight gradient, dx2 data gradient).  The unread channels
           of an input hold NaN, those of an output a sentinel that must survive.
  split    0, or the channels of the first tensor: the *_cat entry points
  bias     False: the NULL pointer (forward);  stats  True: the forward writes the fused statistics partials;  dbias  False: NULL
  passes   which of ("fwd", "dgrad", "wgrad") the row runs
  nums     {pass: {field of ops.conv_mfma_plan, or "route": value}} for both storage types, or {"fwd/f32": ..} for one: the plan
           facts the row is there for (tests/test_mfma_plan.py holds every row to them on the CPU, the GPU test with the real
           pointers).  "route" is the name mri3d_conv3d_route gives.
  refused  {storage type: passes the entry point refuses (route "none")}: MRI3D_ENOTSUP, and nothing written
  leaves   {storage type: passes another file's kernel serves}: the plan query must refuse; the pass is not run here

Kc = input channels of a pass (forward ci, data gradient co), Nc = its output channels.  fp32 thresholds the shapes are chosen by:
plain fp32 reaches the tiled kernels only from 512 work units (n = 64 at 5x9x17: 8 tiles x 64) — below, the direct kernel takes
it —, with fused statistics at any size, with a split operand from 256 units (n = 32); every stride-1 bf16 row is tiled."""
import collections

Row = collections.namedtuple("Row", "id ci co n sp stride layout split bias stats dbias passes nums refused leaves")

DTYPES = ("f32", "bf16")
FD = ("fwd", "dgrad")
ALL = ("fwd", "dgrad", "wgrad")


def row(id_, ci, co, sp, n=1, stride=1, layout=None, split=0, bias=True, stats=False, dbias=True, passes=FD, nums=None, refused=None,
        leaves=None):
    return Row(id_, ci, co, n, tuple(sp), stride, layout or {}, split, bias, stats, dbias, tuple(passes), nums or {}, refused or {},
               leaves or {})


def per(f32=None, bf16=None, passes=FD):
    """{"pass/type": numbers}: the same numbers for each of `passes` in a storage type"""
    out = {}
    for t, d in (("f32", f32), ("bf16", bf16)):
        if d is not None:
            out.update({"%s/%s" % (p, t): dict(d) for p in passes})
    return out


def both(passes=FD, **kw):
    return {p: dict(kw) for p in passes}


def merge(*ds):
    out = {}
    for d in ds:
        for k, v in d.items():
            out.setdefault(k, {}).update(v)
    return out


T1 = dict(kernel="tiled", route="tiled nt1")
T2 = dict(kernel="tiled", route="tiled nt2")
N8 = dict(kernel="tiled_n8", route="tiled_n8")
S1 = dict(kernel="tiled", route="tiled nt1 stats")
S2 = dict(kernel="tiled", route="tiled nt2 stats")
D1 = dict(kernel="direct", route="direct nt1 mode0 split1", nt=1, mode=0, split=1)
W6 = dict(kernel="wgrad6", route="wgrad6", tile_d=2, tile_h=6, tile_w=16, ci8=0, co8=0)
WB = dict(kernel="bf16", route="bf16", tile_d=2, tile_h=6, tile_w=32)
W3 = dict(kernel="wgrad3", route="wgrad3", tile_d=2, tile_h=8, tile_w=16, ck=8, tg=14)
FWD = ("fwd",)
WG = ("wgrad",)

# ---- tiles of the tiled kernels (4 x 8 x 16) and of the weight-gradient kernels; plain fp32 is the direct kernel at these sizes
TILES = [
    row("tile-exact-4x8x16", 16, 16, (4, 8, 16), passes=ALL, nums=merge(
        per(bf16=dict(T1, tiles_d=1, tiles_h=1, tiles_w=1, ntiles=1, grid=1, partial_chunk=0), f32=dict(D1, ntiles=32, units=32, grid=32)),
        {"wgrad/f32": dict(W6, ntiles=4, p=4, max_tasks=1, min_tasks=1, chain=48), "wgrad/bf16": dict(WB, ntiles=4, p=4, chain=96)})),
    # 12 weight-gradient tiles on 12 workgroups, which is no multiple of 8: the XCD ranges are uneven, workgroups get 2, 1 and 0 tiles
    row("tile-ragged-5x9x17", 16, 16, (5, 9, 17), passes=ALL, nums=merge(
        per(bf16=dict(T1, tiles_d=2, tiles_h=2, tiles_w=2, ntiles=8, grid=8, max_tasks=1, min_tasks=1), f32=dict(D1, ntiles=48)),
        {"wgrad/f32": dict(W6, tiles_d=3, tiles_h=2, tiles_w=2, ntiles=12, p=12, max_tasks=2, min_tasks=0, chain=96),
         "wgrad/bf16": dict(WB, tiles_d=3, tiles_h=2, tiles_w=1, ntiles=6, p=6, max_tasks=1, min_tasks=1, chain=96)})),
    row("tile-one-voxel-in-second-w-tile", 16, 16, (4, 8, 17), nums=per(bf16=dict(T1, tiles_w=2, ntiles=2), f32=dict(D1, ntiles=34))),
    # extents below one tile; every tap but the centre one falls outside 1x1x1: 26 exact zeros per (co, ci) of dw
    row("tile-1x1x1", 16, 16, (1, 1, 1), passes=ALL, nums=merge(per(bf16=dict(T1, ntiles=1), f32=dict(D1, ntiles=1, grid=1)),
                                                                 {"wgrad/f32": dict(W6, ntiles=1, p=1, chain=48), "wgrad/bf16": dict(WB, ntiles=1, p=1)})),
    row("tile-3x3x3", 16, 16, (3, 3, 3), passes=ALL, nums=merge(per(bf16=dict(T1, ntiles=1), f32=dict(D1, ntiles=2)),
                                                                 {"wgrad/f32": dict(W6, ntiles=2, p=2), "wgrad/bf16": dict(WB, ntiles=2, p=2)})),
    row("tile-d1-1x8x16", 16, 16, (1, 8, 16), passes=ALL, nums=merge(per(bf16=dict(T1, ntiles=1), f32=dict(D1, ntiles=8)),
                                                                     {"wgrad/f32": dict(W6, tiles_d=1, ntiles=2), "wgrad/bf16": dict(WB, tiles_d=1, ntiles=2)})),
]

# ---- the forward with fused statistics: tiled at every size in both types
STATS = [
    row("stats-exact-4x8x16", 16, 16, (4, 8, 16), stats=True, passes=FWD, nums={"fwd": dict(S1, ntiles=1, grid=1, stats_blocks=1)}),
    row("stats-ragged-5x9x17", 16, 16, (5, 9, 17), stats=True, passes=FWD,
        nums={"fwd": dict(S1, ntiles=8, grid=8, stats_blocks=8), "fwd/f32": dict(ck=8, chunks=2), "fwd/bf16": dict(ck=16, chunks=1)}),
    row("stats-ragged-no-bias", 16, 16, (5, 9, 17), stats=True, bias=False, passes=FWD, nums={"fwd": dict(S1, stats_blocks=8)}),
    row("stats-one-voxel-in-second-w-tile", 16, 16, (4, 8, 17), stats=True, passes=FWD, nums={"fwd": dict(S1, tiles_w=2, ntiles=2)}),
    # at most 8 voxels wide: fp32 has no fused statistics there (the direct kernel's volumes), bf16 has
    row("stats-1x1x1", 16, 16, (1, 1, 1), stats=True, passes=FWD, nums={"fwd/bf16": dict(S1, ntiles=1)}, refused={"f32": FWD}),
    row("stats-3x3x3", 16, 16, (3, 3, 3), stats=True, passes=FWD, nums={"fwd/bf16": dict(S1, ntiles=1)}, refused={"f32": FWD}),
    row("stats-h1-w9", 16, 16, (3, 1, 9), stats=True, passes=FWD, nums={"fwd": dict(S1, ntiles=1)}),
    row("stats-d1-1x8x16", 16, 16, (1, 8, 16), stats=True, passes=FWD, nums={"fwd": dict(S1, ntiles=1)}),
    row("stats-n3", 16, 16, (5, 9, 17), n=3, stats=True, passes=FWD, nums={"fwd": dict(S1, ntiles=24, grid=24, stats_blocks=24)}),
    # 12 units on 12 workgroups: two tiles for some, none for others, whose partials must be zeros
    row("stats-grid12-empty-workgroups", 16, 16, (9, 9, 17), stats=True, passes=FWD,
        nums={"fwd": dict(S1, units=12, grid=12, max_tasks=2, min_tasks=0, stats_blocks=12)}),
    row("stats-kc8", 8, 16, (5, 9, 17), stats=True, passes=FWD, nums={"fwd/f32": dict(S1, chunks=1, partial_chunk=0),
                                                                      "fwd/bf16": dict(S1, chunks=1, partial_chunk=1)}),
    row("stats-kc48", 48, 16, (5, 9, 17), stats=True, passes=FWD, nums={"fwd/f32": dict(S1, chunks=6), "fwd/bf16": dict(S1, chunks=3)}),
    row("stats-nt1-gy3", 16, 48, (5, 9, 17), stats=True, passes=FWD, nums={"fwd": dict(S1, nt=1, ntt=3, gy=3, units=24, grid=24)}),
    row("stats-nt2-gy1", 16, 32, (5, 9, 17), stats=True, passes=FWD, nums={"fwd": dict(S2, nt=2, ntt=2, gy=1, units=8)}),
    row("stats-nt2-gy2", 16, 64, (5, 9, 17), stats=True, passes=FWD, nums={"fwd": dict(S2, nt=2, ntt=4, gy=2, units=16)}),
    row("stats-nc24-half-empty-n-tile", 16, 24, (5, 9, 17), stats=True, passes=FWD, nums={"fwd": dict(S2, nt=2, ntt=2, gy=1)}),
    row("stats-128-channels", 8, 128, (5, 9, 17), stats=True, passes=FWD, nums={"fwd": dict(S2, ntt=8, gy=4, units=32, stats_blocks=32)}),
    row("stats-136-channels-refused", 8, 136, (5, 9, 17), stats=True, passes=FWD, refused={"f32": FWD, "bf16": FWD}),
]

# ---- K chunks: 8 fp32 / 16 bf16 channels (tiled), 16 (direct); bf16 Kc = 8, 24: the last chunk half filled
CHUNKS = [
    row("kc8", 8, 16, (5, 9, 17), passes=ALL, nums={
        "fwd/bf16": dict(T1, ck=16, chunks=1, partial_chunk=1), "dgrad/bf16": dict(N8, chunks=1, partial_chunk=0),
        "fwd/f32": dict(D1, chunks=1, partial_chunk=1), "dgrad/f32": dict(D1, chunks=1, partial_chunk=0),
        "wgrad/f32": dict(W3, cit=1, max_tasks=2, min_tasks=0, chain=128), "wgrad/bf16": dict(WB, cit=1, partial_chunk=1)}),
    row("kc24", 24, 16, (5, 9, 17), passes=ALL, nums={
        "fwd/bf16": dict(T1, chunks=2, partial_chunk=1), "dgrad/bf16": dict(T2, chunks=1, ntt=2),
        "fwd/f32": dict(D1, chunks=2, partial_chunk=1), "dgrad/f32": dict(D1, chunks=1, ntt=2, gy=2, units=96),
        "wgrad/f32": dict(W3, cit=3, grid=36), "wgrad/bf16": dict(WB, cit=2, partial_chunk=1, grid=12)}),
    # the chunk's upper half lies over the NaN of the channels that follow the slice
    row("kc24-x-pitched-nan-behind", 24, 16, (5, 9, 17), passes=ALL, layout={"x": (40, 8)}, nums={
        "fwd/bf16": dict(T1, chunks=2, partial_chunk=1), "fwd/f32": dict(D1, chunks=2, partial_chunk=1),
        "wgrad/f32": dict(W3, cit=3), "wgrad/bf16": dict(WB, cit=2, partial_chunk=1)}),
    row("kc8-x-pitched-1x1x1", 8, 64, (1, 1, 1), layout={"x": (16, 8)}, nums={"fwd/bf16": dict(T2, partial_chunk=1), "fwd/f32": dict(D1)}),
    row("kc8-x-pitched-nan-behind", 8, 16, (5, 9, 17), passes=ALL, layout={"x": (16, 0)}, nums={
        "fwd/bf16": dict(T1, chunks=1, partial_chunk=1), "wgrad/bf16": dict(WB, partial_chunk=1), "wgrad/f32": dict(W3)}),
]

# ---- N-tiles: NT per wave, gy passes; eight output channels
NTILES = [
    row("nt1-gy3", 16, 48, (5, 9, 17), passes=ALL, nums={
        "fwd/bf16": dict(T1, nt=1, ntt=3, gy=3, units=24, grid=24), "dgrad/bf16": dict(T1, chunks=3),
        "fwd/f32": dict(D1, ntt=3, gy=3, units=144), "wgrad/f32": dict(W6, cob=3, grid=36), "wgrad/bf16": dict(WB, cob=3, grid=18)}),
    row("nt2-gy1", 16, 32, (5, 9, 17), nums={"fwd/bf16": dict(T2, nt=2, ntt=2, gy=1, units=8), "fwd/f32": dict(D1, ntt=2, gy=2)}),
    # fp32: four N-tiles would be nt 4; the loop narrows it to 1 for 48 M-tiles
    row("nt2-gy2", 16, 64, (5, 9, 17), nums={"fwd/bf16": dict(T2, nt=2, ntt=4, gy=2, units=16, grid=16),
                                             "fwd/f32": dict(D1, nt=1, ntt=4, gy=4, units=192)}),
    row("nc24-half-empty-n-tile", 16, 24, (5, 9, 17), passes=ALL, nums={
        "fwd/bf16": dict(T2, nt=2, ntt=2), "dgrad/bf16": dict(T1, chunks=2, partial_chunk=1), "fwd/f32": dict(D1, ntt=2),
        "wgrad/f32": dict(W6, cob=2, grid=24), "wgrad/bf16": dict(WB, cob=2, grid=12)}),
    row("nc8", 16, 8, (5, 9, 17), passes=ALL, nums={
        "fwd/bf16": dict(N8), "dgrad/bf16": dict(T1, partial_chunk=1), "fwd/f32": dict(D1, ntt=1), "dgrad/f32": dict(D1, partial_chunk=1),
        "wgrad/f32": dict(kernel="wgrad6", route="wgrad6 co8", ci8=0, co8=1, tg=18), "wgrad/bf16": dict(WB)}),
    row("ci8-co8", 8, 8, (5, 9, 17), passes=ALL, nums={
        "fwd/bf16": dict(N8, partial_chunk=1), "dgrad/bf16": dict(N8, partial_chunk=1), "fwd/f32": dict(D1),
        "wgrad/f32": dict(kernel="wgrad6", route="wgrad6 ci8 co8", ci8=1, co8=1, tg=10), "wgrad/bf16": dict(WB, partial_chunk=1)}),
    row("nc8-n64", 16, 8, (5, 9, 17), n=64, nums={"fwd/f32": dict(N8, ck=8, chunks=2, units=512, grid=512), "dgrad/f32": dict(T1, ck=8, chunks=1),
                                                  "fwd/bf16": dict(N8, grid=512), "dgrad/bf16": dict(T1, partial_chunk=1)}),
    row("ci8-n64", 8, 16, (5, 9, 17), n=64, nums={"fwd/f32": dict(T1, ck=8, chunks=1), "dgrad/f32": dict(N8, ck=8, chunks=2, grid=512),
                                                  "fwd/bf16": dict(T1, partial_chunk=1), "dgrad/bf16": dict(N8)}),
]

# ---- the persistent grid: 512 workgroups at most; plain fp32 is tiled from 512 units
PERSIST = [
    row("n64-512-units", 16, 16, (5, 9, 17), n=64, passes=ALL, nums=merge(
        per(f32=dict(T1, ck=8, chunks=2, units=512, grid=512, max_tasks=1, min_tasks=1), bf16=dict(T1, units=512, grid=512, max_tasks=1)),
        {"wgrad/f32": dict(W6, ntiles=768, p=512, max_tasks=2, min_tasks=1, chain=96),
         "wgrad/bf16": dict(WB, ntiles=384, p=384, max_tasks=1, min_tasks=1, chain=96)})),
    row("n72-second-tile", 16, 16, (5, 9, 17), n=72, nums=both(kernel="tiled", route="tiled nt1", units=576, grid=512, max_tasks=2, min_tasks=1)),
    # grids that are no multiple of 8 (the XCD remap): 12 workgroups take 2, 1 and 0 of 12 tiles
    row("grid12", 16, 16, (9, 9, 17), nums=per(bf16=dict(T1, units=12, grid=12, max_tasks=2, min_tasks=0), f32=dict(D1))),
    row("grid3", 16, 16, (4, 8, 48), nums=per(bf16=dict(T1, units=3, grid=3, max_tasks=1, min_tasks=1), f32=dict(D1))),
]

# ---- split operands (the *_cat entry points): fp32 takes them from 256 units (n = 32 at 5x9x17)
SPLIT = [
    row("split-16+8", 24, 16, (5, 9, 17), n=32, split=16, passes=ALL, refused={"f32": WG}, nums={
        "fwd/f32": dict(T1, chunks=3, units=256), "dgrad/f32": dict(T2, ntt=2), "fwd/bf16": dict(T1, chunks=2, partial_chunk=1),
        "dgrad/bf16": dict(T2), "wgrad/bf16": dict(WB, cit=2, partial_chunk=1)}),
    row("split-16+16", 32, 16, (5, 9, 17), n=32, split=16, passes=ALL, nums={
        "fwd/f32": dict(T1, chunks=4), "dgrad/f32": dict(T2), "fwd/bf16": dict(T1, chunks=2), "dgrad/bf16": dict(T2),
        "wgrad/f32": dict(W6, cit=2, p=256, max_tasks=2, min_tasks=1, chain=96), "wgrad/bf16": dict(WB, cit=2, p=192)}),
    row("split-8+8-refused", 16, 16, (5, 9, 17), n=32, split=8, passes=ALL, refused={"f32": ALL, "bf16": ALL}),
    row("split-16+16-second-pitched-no-dbias", 32, 16, (5, 9, 17), n=32, split=16, passes=ALL, dbias=False, layout={"x2": (24, 8)},
        nums={"fwd": dict(T1), "dgrad": dict(T2), "wgrad/f32": dict(W6), "wgrad/bf16": dict(WB)}),
    # the data gradient writes dx and dx2 into slices of wider buffers
    row("split-16+16-all-pitched", 32, 16, (5, 9, 17), n=32, split=16, passes=ALL, layout={"x": (24, 8), "x2": (24, 8), "y": (24, 8)},
        nums={"fwd": dict(T1), "dgrad": dict(T2), "wgrad/f32": dict(W6), "wgrad/bf16": dict(WB)}),
    row("split-16+16-stats", 32, 16, (5, 9, 17), n=32, split=16, stats=True, passes=FWD, nums={"fwd": dict(S1, grid=256, stats_blocks=256)}),
    # fp32 below 256 units or at most 8 voxels wide: the direct kernel's sizes, and that has no second operand
    row("split-few-units", 32, 16, (5, 9, 17), split=16, passes=ALL, refused={"f32": FD}, nums={
        "fwd/bf16": dict(T1, units=8), "dgrad/bf16": dict(T2), "wgrad/f32": dict(W6, cit=2), "wgrad/bf16": dict(WB, cit=2)}),
    row("split-narrow", 32, 16, (9, 9, 8), n=32, split=16, refused={"f32": FD}, nums={"fwd/bf16": dict(T1, units=192), "dgrad/bf16": dict(T2)}),
]

# ---- the direct kernel at stride 1 (fp32; the bf16 numbers are the tiled kernel's)
DIRECT = [
    row("direct-nt4", 8, 128, (32, 32, 32), passes=FWD, nums={
        "fwd/f32": dict(kernel="direct", route="direct nt4 mode0 split0", nt=4, ntt=8, gy=2, ntiles=2048, units=4096, grid=1024, split=0,
                        partial_chunk=1), "fwd/bf16": dict(T2, units=256)}),
    # four N-tiles, 2048 M-tiles: the loop narrows nt 4 to 2
    row("direct-nt4-narrowed-to-2", 8, 64, (32, 32, 32), passes=FWD, nums={
        "fwd/f32": dict(kernel="direct", route="direct nt2 mode0 split0", nt=2, ntt=4, gy=2, units=4096, split=0)}),
    row("direct-nt2", 8, 96, (28, 28, 28), passes=FWD, nums={
        "fwd/f32": dict(kernel="direct", route="direct nt2 mode0 split0", nt=2, ntt=6, gy=3, ntiles=1372, units=4116, grid=1029, split=0)}),
    row("direct-1023-units", 16, 16, (11, 31, 48), nums=per(f32=dict(D1, units=1023, grid=1023, split=1), bf16=dict(T1, units=36, max_tasks=2, min_tasks=0))),
    row("direct-1024-units", 16, 16, (16, 32, 32), nums=per(
        f32=dict(kernel="direct", route="direct nt1 mode0 split0", units=1024, grid=256, split=0), bf16=dict(T1, units=32))),
    row("direct-narrow-w8", 16, 16, (8, 8, 8), n=2, nums=per(f32=dict(D1, ntiles=64), bf16=dict(T1, ntiles=4))),
    # 45 voxels a sample: M-tiles span rows, planes and the two samples, the last one is ragged
    row("direct-odd-voxel-count", 16, 16, (3, 3, 5), n=2, nums=per(f32=dict(D1, ntiles=6, units=6), bf16=dict(T1, ntiles=2))),
]

# ---- strides 2 and 3: the direct kernel in both storage types, mode 0 forward, mode 1 data gradient (M-tiles per row residue)
M1 = dict(kernel="direct", route="direct nt1 mode1 split1", mode=1, split=1)
STRIDED = [
    row("s2-even-extents", 16, 16, (8, 8, 16), stride=2, passes=ALL, leaves={"f32": WG, "bf16": WG},
        nums={"fwd": dict(D1, ntiles=8), "dgrad": dict(M1, ntiles=128, wbn=1)}),
    row("s2-odd-extents-kc12", 12, 16, (5, 9, 37), stride=2, nums={"fwd": dict(D1, chunks=1, partial_chunk=1, ntiles=18),
                                                                  "dgrad": dict(M1, wbn=2, ntiles=180)}),
    row("s3-kc20", 20, 16, (7, 9, 50), stride=3, nums={"fwd": dict(D1, chunks=2, partial_chunk=1, ntiles=10),
                                                       "dgrad": dict(M1, wbn=2, ntt=2, gy=2, ntiles=378, units=756)}),
    row("s2-nc8", 16, 8, (6, 7, 9), stride=2, nums={"fwd": dict(D1, ntt=1, ntiles=4), "dgrad": dict(M1, partial_chunk=1, ntiles=84)}),
    # nt 2 and 4 need 4096 units (and then the waves are not split): the smallest strided volumes that have them
    row("s2-fwd-nt2-dgrad-split0", 8, 32, (64, 64, 128), stride=2, nums={
        "fwd": dict(kernel="direct", route="direct nt2 mode0 split0", nt=2, ntt=2, gy=1, units=4096, grid=1024),
        "dgrad": dict(kernel="direct", route="direct nt1 mode1 split0", nt=1, wbn=4, units=32768, grid=8192)}),
    row("s2-fwd-nt4", 8, 64, (64, 64, 128), stride=2, passes=FWD, nums={
        "fwd": dict(kernel="direct", route="direct nt4 mode0 split0", nt=4, ntt=4, gy=1, units=4096)}),
    row("s2-fwd-split0", 8, 16, (32, 64, 64), stride=2, passes=FWD, nums={
        "fwd": dict(kernel="direct", route="direct nt1 mode0 split0", nt=1, units=1024, grid=256, split=0)}),
    row("s2-dgrad-nt2", 32, 8, (32, 32, 64), stride=2, passes=("dgrad",), nums={
        "dgrad": dict(kernel="direct", route="direct nt2 mode1 split0", nt=2, ntt=2, gy=1, wbn=2, units=4096)}),
    row("s2-dgrad-nt4", 64, 8, (32, 32, 64), stride=2, passes=("dgrad",), nums={
        "dgrad": dict(kernel="direct", route="direct nt4 mode1 split0", nt=4, ntt=4, gy=1, units=4096)}),
]

# ---- the weight-gradient kernels and their workgroup walk
WGRAD = [
    row("wg-cin1", 1, 16, (5, 9, 17), passes=WG, nums={"wgrad": dict(kernel="cin1", route="cin1", ck=1, tg=2, ntiles=12, p=12, max_tasks=1, chain=64)}),
    row("wg-cin1-two-tiles", 1, 16, (5, 9, 17), n=48, passes=WG, nums={"wgrad": dict(kernel="cin1", route="cin1", ntiles=576, p=512, max_tasks=2,
                                                                                     min_tasks=1, chain=128)}),
    row("wg3-ci8-co12", 8, 12, (5, 9, 17), passes=WG, nums={"wgrad": dict(W3, cit=1, max_tasks=2, min_tasks=0, chain=128)}),
    row("wg3-ci24-co12-no-dbias", 24, 12, (5, 9, 17), passes=WG, dbias=False, nums={"wgrad": dict(W3, cit=3, grid=36)}),
    # bf16 tensors the bf16 MFMA kernels cannot take: co % 8 != 0, or a pitch % 8 != 0
    row("wg4-co12", 16, 12, (5, 9, 17), passes=WG, nums={
        "wgrad/bf16": dict(kernel="wgrad4", route="wgrad4", tile_d=2, tile_h=4, tile_w=16, ntiles=18, p=18, max_tasks=2, min_tasks=0, chain=64),
        "wgrad/f32": dict(W6)}),
    row("wg4-y-pitch-20", 16, 16, (5, 9, 17), passes=WG, layout={"y": (20, 0)}, nums={"wgrad/bf16": dict(kernel="wgrad4", route="wgrad4"),
                                                                                     "wgrad/f32": dict(W6)}),
    row("wg6-cit2", 32, 16, (5, 9, 17), passes=WG, nums={"wgrad/f32": dict(W6, cit=2, grid=24), "wgrad/bf16": dict(WB, cit=2, grid=12)}),
    # P < ntiles with an uneven number of tiles per workgroup
    row("wg-n100-uneven-walk", 16, 16, (5, 9, 17), n=100, passes=WG, nums={
        "wgrad/f32": dict(W6, ntiles=1200, p=512, max_tasks=3, min_tasks=2, chain=144),
        "wgrad/bf16": dict(WB, ntiles=600, p=512, max_tasks=2, min_tasks=1, chain=192)}),
    # bf16t: columns of 8 rows x 32 voxels marching through segments of d; fp32 walks 21 / 12 tiles per workgroup on the same shapes
    row("bf16t-segl20-last-segment-1-plane-no-dbias", 16, 16, (41, 2, 3), n=512, passes=WG, dbias=False, nums={
        "wgrad/bf16": dict(kernel="bf16t", route="bf16t", segl=20, tile_d=20, tile_h=8, tile_w=32, tiles_d=3, ntiles=1536, p=512, max_tasks=3,
                           min_tasks=3, chain=3840), "wgrad/f32": dict(W6, ntiles=10752, max_tasks=21, chain=1008)}),
    row("bf16t-segl40-d8", 16, 16, (8, 2, 3), n=1536, passes=WG, nums={
        "wgrad/bf16": dict(kernel="bf16t", route="bf16t", segl=40, tiles_d=1, ntiles=1536, p=512, max_tasks=3, chain=7680),
        "wgrad/f32": dict(W6, max_tasks=12, chain=576)}),
    row("bf16t-64-64-uneven-walk", 64, 64, (41, 2, 3), n=40, passes=WG, nums={
        "wgrad/bf16": dict(kernel="bf16t", route="bf16t", segl=20, cit=4, cob=4, p=32, ntiles=120, max_tasks=4, min_tasks=3),
        "wgrad/f32": dict(W6, cit=4, cob=4, p=32, max_tasks=27, min_tasks=26)}),
    row("bf16t-split-16+16", 32, 16, (8, 2, 3), n=768, split=16, passes=WG, nums={"wgrad/bf16": dict(kernel="bf16t", route="bf16t", cit=2),
                                                                                 "wgrad/f32": dict(W6, cit=2)}),
]

# ---- x, y / dy as channel slices of wider buffers (16-byte aligned), and slices that are not: those leave the family
LAYOUTS = [
    row("x-pitched", 16, 16, (5, 9, 17), passes=ALL, layout={"x": (24, 8)}, nums=merge(per(f32=D1, bf16=T1), {"wgrad/f32": W6, "wgrad/bf16": WB})),
    row("y-pitched", 16, 16, (5, 9, 17), passes=ALL, layout={"y": (24, 8)}, nums=merge(per(f32=D1, bf16=T1), {"wgrad/f32": W6, "wgrad/bf16": WB})),
    row("x-and-y-pitched-n64", 16, 16, (5, 9, 17), n=64, passes=ALL, layout={"x": (24, 8), "y": (24, 8)},
        nums=merge(per(f32=T1, bf16=T1), {"wgrad/f32": W6, "wgrad/bf16": WB})),
    row("nc8-pitched", 16, 8, (5, 9, 17), n=64, layout={"x": (24, 8), "y": (16, 8)}, nums={"fwd": dict(N8), "dgrad": dict(T1)}),
    row("s2-pitched", 16, 16, (5, 9, 37), stride=2, layout={"x": (24, 8), "y": (24, 8)}, nums={"fwd": dict(D1), "dgrad": dict(M1)}),
    # a slice 8 bytes (fp32) / 4 bytes (bf16) off the 16-byte alignment: the generic kernels take the call
    row("misaligned-x", 16, 16, (5, 9, 17), passes=ALL, layout={"x": (24, 2)}, leaves={"f32": ALL, "bf16": ALL}),
    row("misaligned-y-n64", 16, 16, (5, 9, 17), n=64, passes=ALL, layout={"y": (24, 2)}, leaves={"f32": ALL, "bf16": ALL}),
    row("misaligned-nc8-n64", 16, 8, (5, 9, 17), n=64, passes=ALL, layout={"y": (16, 2)}, leaves={"f32": ALL, "bf16": ALL}),
    row("misaligned-wg3", 8, 12, (5, 9, 17), passes=WG, layout={"x": (16, 2)}, leaves={"f32": WG, "bf16": WG}),
    row("misaligned-wg4", 16, 12, (5, 9, 17), passes=WG, layout={"x": (24, 2)}, leaves={"f32": WG, "bf16": WG}),
    row("misaligned-cin1", 1, 16, (5, 9, 17), passes=WG, layout={"y": (24, 2)}, leaves={"f32": WG, "bf16": WG}),
    row("misaligned-bf16t", 16, 16, (8, 2, 3), n=1536, passes=WG, layout={"y": (24, 2)}, leaves={"f32": WG, "bf16": WG}),
    row("misaligned-s2", 16, 16, (8, 8, 16), stride=2, layout={"x": (24, 2)}, leaves={"f32": FD, "bf16": FD}),
    row("misaligned-x2-split", 32, 16, (5, 9, 17), n=32, split=16, passes=ALL, layout={"x2": (24, 2)}, refused={"f32": ALL, "bf16": ALL}),
]

ROWS = TILES + STATS + CHUNKS + NTILES + PERSIST + SPLIT + DIRECT + STRIDED + WGRAD + LAYOUTS
assert len({r.id for r in ROWS}) == len(ROWS)

PAIRS = [(r, d) for r in ROWS for d in DTYPES]
IDS = ["%s-%s" % (r.id, d) for r, d in PAIRS]


def declared(r, dtype):
    """{pass: {field: value}} the row declares for the storage type"""
    out = {}
    for key, d in r.nums.items():
        p, _, t = key.partition("/")
        if not t or t == dtype:
            out.setdefault(p, {}).update(d)
    return out


def runs(r, dtype, p):
    """the pass is one of the row's and a kernel of the family serves it in this type"""
    return p in r.passes and p not in r.refused.get(dtype, ()) and p not in r.leaves.get(dtype, ())
