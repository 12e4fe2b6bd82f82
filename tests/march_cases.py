"""Rows of the marching-kernel parity suite (tests/test_march_parity_gpu.py; their meaning: tests/march_run.py): Conv3d 3x3x3 /
stride 1 / padding 1 forward and data gradient through mri3d_conv3d_fwd_march / mri3d_conv3d_dgrad_march (csrc/conv_march.hip).

  id       what the row is there for
  ci, co   channels;  n  batch;  sp  extents (D, H, W)
  layout   {"x" | "y" | "x2": (channels of the wider buffer, first channel of the slice)}: x also places dx, y also places dy,
           x2 places the second tensor of a split operand (x2 forward, dx2 data gradient)
  split    0, or the channels of the first tensor: the forward reads cat((x, x2)), the data gradient writes (dx | dx2)
  bias     False: the NULL pointer (forward);  stats  True: the forward writes the fused statistics partials
  passes   which of ("fwd", "dgrad") the row runs
  nums     {"fwd" | "dgrad": {field of ops.conv_march_plan: value}} for both storage types, or {"fwd/f32": ..} for one: the
           plan numbers the row is there for (tests/test_march_plan.py holds every row to them on the CPU)
  refused  {storage type: passes the plan refuses}: there the entry point must return MRI3D_ENOTSUP and write nothing

Kc = input channels of a pass (forward ci, data gradient co), Nc = its output channels.  A chunk holds 8 fp32 / 16 bf16 channels."""
import collections

Row = collections.namedtuple("Row", "id ci co n sp layout split bias stats passes nums refused")

DTYPES = ("f32", "bf16")
BOTH = ("fwd", "dgrad")


def row(id_, ci, co, sp, n=1, layout=None, split=0, bias=True, stats=False, passes=BOTH, nums=None, refused=None):
    return Row(id_, ci, co, n, tuple(sp), layout or {}, split, bias, stats, tuple(passes), nums or {}, refused or {})


def both(**kw):
    return {"fwd": dict(kw), "dgrad": dict(kw)}


DEPTH = [
    row("d1", 16, 16, (1, 8, 16), nums=both(nseg=1, seglen=1, grid=1)),
    row("d2", 16, 16, (2, 8, 16), nums=both(nseg=1, seglen=2, grid=1)),
    row("d3", 16, 16, (3, 8, 16), nums=both(nseg=1, seglen=3, grid=1)),
    # one column: seven of the eight waves are inactive
    row("one-column-d5", 16, 16, (5, 8, 16), nums=both(gch=1, gcw=1, nseg=1, seglen=5, grid=1, blocks=1)),
]

SHAPES = [
    row("wg-4x2", 16, 16, (4, 32, 32), nums=both(wgh=4, wgw=2, gch=1, gcw=1, grid=1)),
    row("wg-2x4", 16, 16, (4, 16, 64), nums=both(wgh=2, wgw=4, gch=1, gcw=1, grid=1)),
    row("wg-8x1-gch2", 16, 16, (4, 70, 8), nums=both(wgh=8, wgw=1, gch=2, gcw=1, grid=2)),
    row("wg-1x8-gcw2-ragged-ninth-column", 16, 16, (3, 5, 130), nums=both(wgh=1, wgw=8, gch=1, gcw=2, grid=2)),
]

# the second and later segments start their march at input plane dlo - 1: residues 1 (7), 2 (8, 17), 0 (15) mod 3 of the tap rotation
SEGMENTS = [
    row("seg-d16-2x8", 16, 16, (16, 8, 16), nums=both(nseg=2, seglen=8, grid=2)),
    row("seg-d25-3x9-last7", 16, 16, (25, 8, 16), nums=both(nseg=3, seglen=9, grid=3)),
    row("seg-d26-3x9-last8-grid3", 16, 16, (26, 8, 16), nums=both(nseg=3, seglen=9, grid=3)),
    row("seg-d40-5x8", 16, 16, (40, 3, 5), nums=both(nseg=5, seglen=8, grid=5)),
]

# {one chunk: 3 buffers, the DMA two items ahead | more chunks: 2 buffers} x {H a multiple of 8 | ragged: no store counted}, D >= 4.
# 8 -> 8 is one chunk in both types, 32 -> 32 four (fp32) and two (bf16); 16 -> 16 (one-column-d5, templates) two and one.
WAITS = [
    row("wait-one-chunk-h8", 8, 8, (5, 8, 16), nums=both(chunks=1, nbuf=3)),
    row("wait-one-chunk-ragged-h", 8, 8, (5, 11, 16), nums=both(chunks=1, nbuf=3)),
    row("wait-chunks-h8", 32, 32, (5, 8, 16), nums={"fwd/f32": dict(chunks=4, nbuf=2), "fwd/bf16": dict(chunks=2, nbuf=2),
                                                    "dgrad/f32": dict(chunks=4, nbuf=2), "dgrad/bf16": dict(chunks=2, nbuf=2)}),
    row("wait-chunks-ragged-h", 32, 32, (5, 11, 16), nums=both(nbuf=2)),
    row("wait-16-16-ragged-h", 16, 16, (5, 11, 16), nums={"fwd/f32": dict(chunks=2, nbuf=2), "fwd/bf16": dict(chunks=1, nbuf=3)}),
]

# Kc of the forward: fp32 8, 16, 24, 32 = 1 .. 4 chunks (40: five, refused); bf16 8 (half a chunk), 16, 24, 56 (four, the last half
# filled), 64 (72: five, refused)
CHUNKS = [
    row("kc8", 8, 16, (4, 9, 17), nums={"fwd/f32": dict(chunks=1, whole_chunks=1), "fwd/bf16": dict(chunks=1, whole_chunks=0)}),
    row("kc24", 24, 16, (4, 9, 17), nums={"fwd/f32": dict(chunks=3, whole_chunks=1), "fwd/bf16": dict(chunks=2, whole_chunks=0)}),
    row("kc32", 32, 16, (4, 9, 17), nums={"fwd/f32": dict(chunks=4), "fwd/bf16": dict(chunks=2, whole_chunks=1)}),
    row("kc40-f32-refused", 40, 16, (4, 9, 17), passes=("fwd",), nums={"fwd/bf16": dict(chunks=3, whole_chunks=0)},
        refused={"f32": ("fwd",)}),
    row("kc56-bf16", 56, 16, (4, 9, 17), passes=("fwd",), nums={"fwd/bf16": dict(chunks=4, whole_chunks=0)}, refused={"f32": ("fwd",)}),
    row("kc64-bf16", 64, 16, (4, 9, 17), passes=("fwd",), nums={"fwd/bf16": dict(chunks=4, whole_chunks=1)}, refused={"f32": ("fwd",)}),
    row("kc72-refused", 72, 16, (4, 9, 17), passes=("fwd",), refused={"f32": ("fwd",), "bf16": ("fwd",)}),
]

OUTPUTS = [
    row("nc8", 16, 8, (4, 9, 17), nums={"fwd": dict(blocks=1)}),
    # fp32 stores whole quads: 12 and 20 channels end inside a block (bf16 stores octets and refuses; Kc = 12, 20 is no data gradient)
    row("nc12-f32", 16, 12, (4, 9, 17), passes=("fwd",), nums={"fwd/f32": dict(blocks=1)}, refused={"bf16": ("fwd",)}),
    row("nc20-f32", 16, 20, (4, 9, 17), passes=("fwd",), nums={"fwd/f32": dict(blocks=2)}, refused={"bf16": ("fwd",)}),
    row("nc24", 16, 24, (4, 9, 17), nums={"fwd": dict(blocks=2)}),
    row("nc48", 16, 48, (4, 9, 17), nums={"fwd": dict(blocks=3, grid=3)}, refused={"f32": ("dgrad",)}),      # Kc = 48: six fp32 chunks
    row("stats-8-blocks", 8, 128, (2, 8, 16), stats=True, passes=("fwd",), nums={"fwd": dict(blocks=8, grid=8)}),
    row("stats-9-blocks-refused", 8, 136, (2, 8, 16), stats=True, passes=("fwd",), refused={"f32": ("fwd",), "bf16": ("fwd",)}),
]

# the whole decode of the remapped workgroup id: output block, segment and sample all above 1; a grid that is no multiple of 8 is
# seg-d26-3x9-last8-grid3 (and the grids of 2, 3 and 5 above)
DECODE = [
    row("decode-n2-2blocks-2seg", 32, 24, (17, 9, 17), n=2, nums={"fwd": dict(blocks=2, nseg=2, seglen=9, grid=8, wgh=4, wgw=2),
                                                                  "dgrad": dict(blocks=2, nseg=2, seglen=9, grid=8)}),
    row("decode-n3-stats", 16, 16, (9, 11, 21), n=3, stats=True, nums={"fwd": dict(grid=3)}),
    # 9 workgroups: the remap hands one of the eight XCD groups two ids, the others one
    row("decode-grid9-n3-3blocks", 16, 48, (3, 8, 16), n=3, passes=("fwd",), nums={"fwd": dict(blocks=3, grid=9)}),
]

OPERANDS = [
    row("x-pitch+8-from-ch8", 16, 16, (4, 9, 17), layout={"x": (24, 8)}),
    row("y-pitch+8-from-ch8", 16, 16, (4, 9, 17), layout={"y": (24, 8)}),
    row("x-and-y-pitched", 16, 16, (4, 9, 17), layout={"x": (24, 8), "y": (24, 8)}),
    # bf16: half a chunk out of a pitched buffer, the upper half of the chunk lies over the next voxel's unread channels
    row("half-chunk-x-pitched", 8, 16, (4, 9, 17), layout={"x": (16, 8)}, nums={"fwd/bf16": dict(whole_chunks=0)}),
    row("kc24-x-and-y-pitched", 24, 24, (4, 9, 17), layout={"x": (32, 8), "y": (32, 8)}),
]

SPLIT = [
    # bf16: the second tensor is half a chunk, on the DMA path that forms its offsets per piece
    row("split-16+8", 24, 16, (4, 9, 17), split=16),
    row("split-16+16", 32, 16, (4, 9, 17), split=16),
    row("split-16+32-bf16", 48, 16, (4, 9, 17), split=16, nums={"fwd/bf16": dict(chunks=3, whole_chunks=1)}, refused={"f32": ("fwd",)}),
    row("split-16+8-second-pitched", 24, 16, (4, 9, 17), split=16, layout={"x2": (16, 8)}),
    row("split-16+16-all-pitched", 32, 16, (4, 9, 17), split=16, layout={"x": (24, 8), "x2": (24, 8), "y": (24, 8)}),
    row("split-16+16-stats", 32, 16, (6, 13, 21), n=2, split=16, stats=True, passes=("fwd",)),
]

# the four kernels {statistics} x {bias} of each type on a volume ragged in H and W (the data gradient has neither: run once)
TEMPLATES = [
    row("tmpl-plain", 16, 16, (11, 13, 37), bias=False, nums=both(wgh=2, wgw=4, gch=1, gcw=1)),
    row("tmpl-bias", 16, 16, (11, 13, 37), passes=("fwd",)),
    row("tmpl-stats", 16, 16, (11, 13, 37), bias=False, stats=True, passes=("fwd",)),
    row("tmpl-stats-bias", 16, 16, (11, 13, 37), stats=True, passes=("fwd",)),
]

ROWS = DEPTH + SHAPES + SEGMENTS + WAITS + CHUNKS + OUTPUTS + DECODE + OPERANDS + SPLIT + TEMPLATES
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
    """the pass is one of the row's and the plan takes it in this type"""
    return p in r.passes and p not in r.refused.get(dtype, ())
