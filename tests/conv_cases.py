"""The convolution case tables of the GPU parity tests, each with the kernel route it exists for.

A table is there for a kernel: its shapes were chosen so that the dispatcher sends them to that kernel.  The dispatcher's answer is
a host decision (`ops.conv_route` -> mri3d_conv3d_route), so tests/test_conv_routes.py checks on the CPU that every case still
reaches the route its table declares, that every route the dispatcher can name has a parity case, and the GPU tests assert the
same route with the real pointers before they launch.  A threshold that moves makes these fail by name instead of silently
moving the cases to another kernel.

`expect[dtype][pass]` is a route name or the leading words of one ("tiled" matches "tiled nt2 stats", not "tiled_n8"); a tuple
holds one entry per case for tables that span several kernels on purpose (the first word of a name is the kernel file: "generic"
matches every kernel of conv_generic.hip).  Passes: "fwd", "dgrad", "wgrad", and "stats" (the
forward with fused BatchNorm statistics) where the test uses it.  Route names: include/mri3d.h at mri3d_conv3d_route.
"""
import numpy as np

from mri_epilepsy_diagnosis_amd import ops
from mri_epilepsy_diagnosis_amd._lib import BF16, F32, PASS_DGRAD, PASS_FWD, PASS_WGRAD

DTYPES = {"f32": F32, "bf16": BF16}
ESIZE = {"f32": 4, "bf16": 2}
PASSES = ("fwd", "dgrad", "wgrad", "stats")


def align_of(byte_offset):
    """Alignment (largest power of two <= 16) of a channel slice that starts `byte_offset` bytes into an allocation."""
    bits = 16 | int(byte_offset)
    return bits & -bits


def matches(name, expected):
    """`expected` is the route name or its leading words."""
    return name == expected or name.startswith(expected + " ")


class Table:
    """cases: the tuples the GPU test is parametrised with; kind: how that test lays its buffers out (`routes` below); oracle: the
    test compares with a torch-CPU reference of the same operation through the plain entry points (what the coverage matrix asks
    for); stride: of the "slice" kind."""

    def __init__(self, name, kind, cases, expect, dtypes=("f32", "bf16"), stride=1, bias=True, oracle=True, ids=None):
        self.name, self.kind, self.cases, self.expect, self.dtypes, self.stride, self.oracle = name, kind, cases, expect, dtypes, stride, oracle
        self.bias = bias
        self.ids = ids if ids is not None else (lambda c: "n%d_%d-%d_%dx%dx%d_p%d_%d" % c[:8])
        assert sorted(expect) == sorted(dtypes), name
        TABLES[name] = self

    def expected(self, case, dtype):
        """[(pass, expected route)]: what the table is there for (`expect`), then the case's own row of PER_CASE."""
        out = []
        for p, e in self.expect[dtype].items():      # (a tuple: one entry per case of this dtype, in table order)
            out.append((p, e[[c for c, dt in pairs(self) if dt == dtype].index(case)] if isinstance(e, tuple) else e))
        row = PER_CASE[(self.name, dtype)][self.ids(case)].split(" | ")
        assert len(row) == len(ORDER[self.kind]), (self.name, dtype, self.ids(case))
        return out + list(zip(ORDER[self.kind], row))

    def routes(self, case, dtype, x_align=None, dy_align=None):
        """{pass: route name} of a case as its GPU test runs it; the alignments default to those the test's layout gives slices
        of freshly allocated buffers."""
        return ROUTES[self.kind](self, case, dtype, x_align, dy_align)

    def shape(self, case, pass_="fwd"):
        """(n, d, h, w) of the input volume ("transpose": of the volume the pass's kernel walks — the output in the forward, the
        input in the gradients)."""
        if self.kind == "transpose" and pass_ != "fwd":
            return (case[0],) + tuple(case[3])
        return SHAPES[self.kind](case)

    def check(self, case, dtype, x=None, dy=None):
        """Assert the declared routes; with the test's real tensors (x: the input slice, dy: the incoming gradient) the query
        sees their actual base addresses."""
        xa = None if x is None else ops._ptr_align(x)
        da = None if dy is None else ops._ptr_align(dy)
        got = self.routes(case, dtype, xa, da)
        wrong = sorted({"%s %s %s %s: the dispatcher routes to '%s', the table is there for '%s'" % (self.name, self.ids(case), dtype, p, got[p], e)
                        for p, e in self.expected(case, dtype) if not matches(got[p], e)})
        assert not wrong, "\n  ".join(wrong)
        return got


TABLES = {}
PER_CASE = {}       # (table name, dtype) -> {case id: "route | route | ..." in the order ORDER[kind]}; at the end of this file


def is_ragged(n, d, h, w):
    """Ragged in d, h and w for every tile shape in use: all three extents odd (the tiles' extents are even) and above one."""
    return d > 1 and h > 1 and w > 1 and d % 2 == 1 and h % 2 == 1 and w % 2 == 1


# ---- "slice": (nb, ci, co, d, h, w, pad_in, pad_out, seed) of test_fuzz_gpu._run_conv_case — 3x3x3, pad 1, with a bias; x is channels
# [pad_in, pad_in + ci) of a buffer of pitch ci + pad_in, the incoming gradient channels [0, co) of one of pitch co + pad_out
def _slice_routes(t, case, dtype, x_align, dy_align):
    nb, ci, co, d, h, w, pad_in, pad_out = case[:8]
    if x_align is None:
        x_align = align_of(pad_in * ESIZE[dtype])
    return ops.conv3d_routes((nb, ci, d, h, w), (co, ci, 3, 3, 3), t.stride, 1, 1, DTYPES[dtype], x_ld=ci + pad_in, dy_ld=co + pad_out,
                             bias=t.bias, x_align=x_align, dy_align=16 if dy_align is None else dy_align)


# ---- "first": (nb, co, d, h, w, bias, pad_out) of test_first_layer_conv_one_input_channel — one input channel, dense x; the
# incoming gradient is channels [pad_out, pad_out + co) of a buffer of pitch co + pad_out
def _first_routes(t, case, dtype, x_align, dy_align):
    nb, co, d, h, w, bias, pad_out = case
    if dy_align is None:
        dy_align = align_of(pad_out * ESIZE[dtype])
    return ops.conv3d_routes((nb, 1, d, h, w), (co, 1, 3, 3, 3), 1, 1, 1, DTYPES[dtype], dy_ld=co + pad_out, bias=bias,
                             x_align=16 if x_align is None else x_align, dy_align=dy_align)


# ---- "dense": dense tensors, any kernel / stride / padding / dilation; `t.fields(case)` -> (n, ci, co, (d, h, w), k, s, p, dil, bias)
def _dense_routes(t, case, dtype, x_align, dy_align):
    n, ci, co, sp, k, s, p, dil, bias = t.fields(case)
    k = ops._triple(k)
    return ops.conv3d_routes((n, ci) + tuple(sp), (co, ci) + k, s, p, dil, DTYPES[dtype], bias=bias,
                             x_align=16 if x_align is None else x_align, dy_align=16 if dy_align is None else dy_align)


# ---- "stats": (nb, ci, co, d, h, w, has_bias) of the fused-statistics test in test_ops_gpu — dense, run with and without bn_stats
def _stats_routes(t, case, dtype, x_align, dy_align):
    nb, ci, co, d, h, w, bias = case
    kw = dict(bias=bias, x_align=16 if x_align is None else x_align, dy_align=16 if dy_align is None else dy_align)
    r = ops.conv3d_routes((nb, ci, d, h, w), (co, ci, 3, 3, 3), 1, 1, 1, DTYPES[dtype], **kw)
    r["stats"] = ops.conv3d_routes((nb, ci, d, h, w), (co, ci, 3, 3, 3), 1, 1, 1, DTYPES[dtype], bn_stats=True, **kw)["fwd"]
    return r


# ---- "cat": (nb, ca, cb, co, (d, h, w), pad_b, bias, served in fp32, served in bf16) of the split-operand test in test_ops_gpu: the
# second tensor is channels [pad_b, pad_b + cb) of a buffer of pitch cb + pad_b; the gradient comes back as two dense tensors
def _cat_routes(t, case, dtype, x_align, dy_align):
    nb, ca, cb, co, sp, pad_b, bias = case[:7]
    shape, wshape, one = (nb, ca + cb) + tuple(sp), (co, ca + cb, 3, 3, 3), (1, 1, 1)
    align = align_of(pad_b * ESIZE[dtype]) if x_align is None else x_align
    gf = ops._conv_geom(shape, wshape, one, one, one, x_ld=ca, dtype=DTYPES[dtype])
    return {"fwd": ops.conv_route(gf, PASS_FWD, False, bias, ca, cb + pad_b, align),
            "stats": ops.conv_route(gf, PASS_FWD, True, bias, ca, cb + pad_b, align),
            "dgrad": ops.conv_route(gf, PASS_DGRAD, False, False, ca, cb, 16),
            "wgrad": ops.conv_route(gf, PASS_WGRAD, False, False, ca, cb + pad_b, align)}


# ---- "capi_stats": (id, dtype, n, ca, cb, second-tensor pitch, co, volume, kernel-name pattern) of test_buffer_contracts_gpu: the
# fused-statistics forward through the C ABI, one tensor (cb == 0) or a split operand whose second tensor ends its buffer
def _capi_stats_routes(t, case, dtype, x_align, dy_align):
    cid, _, n, ca, cb, ld2, co, sp, _ = case
    one = (1, 1, 1)
    g = ops._conv_geom((n, ca + cb) + tuple(sp), (co, ca + cb, 3, 3, 3), one, one, one, x_ld=ca, dtype=DTYPES[dtype])
    align = align_of((ld2 - cb) * ESIZE[dtype]) if x_align is None else x_align
    return {"stats": ops.conv_route(g, PASS_FWD, True, True, ca if cb else 0, ld2, align)}


# ---- "stats_fwd": (nb, ci, co, d, h, w, has_bias) of test_fuzz_gpu's fused-statistics oracle test: the forward only, dense
def _stats_fwd_routes(t, case, dtype, x_align, dy_align):
    return {"stats": _stats_routes(t, case, dtype, x_align, dy_align)["stats"]}


# ---- "geom": (n, ci, co, (d, h, w), k, stride, padding, dilation, bias, pad_in, pad_out) of tests/test_conv_variants_gpu.py — any filter;
# x is channels [pad_in, pad_in + ci) of a buffer of pitch ci + pad_in, the incoming gradient channels [pad_out, pad_out + co) of one
# of pitch co + pad_out (pads 0 / 0: dense); the other channels of both buffers hold a sentinel
def _geom_routes(t, case, dtype, x_align, dy_align):
    n, ci, co, sp, k, s, p, dil, bias, pad_in, pad_out = case
    if x_align is None:
        x_align = align_of(pad_in * ESIZE[dtype])
    if dy_align is None:
        dy_align = align_of(pad_out * ESIZE[dtype])
    return ops.conv3d_routes((n, ci) + tuple(sp), (co, ci) + tuple(k), s, p, dil, DTYPES[dtype], x_ld=ci + pad_in, dy_ld=co + pad_out, bias=bias,
                             x_align=x_align, dy_align=dy_align)


# ---- "transpose": (n, ci, co, (d, h, w), k, stride, padding, output_padding, bias) of ConvTranspose3d(ci, co, ...) on dense tensors.  The
# routes are those of the mirrored convolution `_ConvTranspose3dFn` builds: "fwd" is its data gradient WITH the bias, "dgrad" its
# forward without one, "wgrad" its weight gradient with the operands swapped.  The volume a case counts as ragged by is the
# transposed convolution's OUTPUT (what the forward's data-gradient kernel walks)
def _transpose_routes(t, case, dtype, x_align, dy_align):
    n, ci, co, sp, k, s, p, op, bias = case
    return ops.conv_transpose3d_routes((n, ci) + tuple(sp), (ci, co) + tuple(k), s, p, op, 1, DTYPES[dtype], bias,
                                       x_align=16 if x_align is None else x_align, dy_align=16 if dy_align is None else dy_align)


# ---- "ws_wgrad": (id, dtype, "geom" case, channel offset of the incoming gradient in its buffer, seed, kernel-name pattern) of the
# exact-workspace test in test_buffer_contracts_gpu: as "geom", but the incoming gradient is channels [dy_off, dy_off + co) of its
# buffer of pitch co + pad_out, so that it can be misaligned under a pitch that is a multiple of 4
def _ws_wgrad_routes(t, case, dtype, x_align, dy_align):
    if dy_align is None:
        dy_align = align_of(case[3] * ESIZE[dtype])
    return _geom_routes(t, case[2], dtype, x_align, dy_align)


# pass of the mirrored convolution whose kernel runs in each pass of the transposed one
KERNEL_PASS = {"transpose": {"fwd": "dgrad", "dgrad": "fwd", "wgrad": "wgrad"}}


def transpose_out(case):
    n, ci, co, sp, k, s, p, op, bias = case
    return tuple((i - 1) * ss - 2 * pp + (kk - 1) + oo + 1 for i, ss, pp, kk, oo in zip(sp, s, p, k, op))


ORDER = {"slice": ("fwd", "dgrad", "wgrad"), "first": ("fwd", "dgrad", "wgrad"), "dense": ("fwd", "dgrad", "wgrad"),
         "stats": ("fwd", "dgrad", "wgrad", "stats"), "cat": ("fwd", "stats", "dgrad", "wgrad"), "capi_stats": ("stats",), "stats_fwd": ("stats",),
         "geom": ("fwd", "dgrad", "wgrad"), "transpose": ("fwd", "dgrad", "wgrad"), "ws_wgrad": ("fwd", "dgrad", "wgrad")}
ROUTES = {"slice": _slice_routes, "first": _first_routes, "dense": _dense_routes, "stats": _stats_routes, "cat": _cat_routes,
          "capi_stats": _capi_stats_routes, "stats_fwd": _stats_fwd_routes, "geom": _geom_routes, "transpose": _transpose_routes,
          "ws_wgrad": _ws_wgrad_routes}
SHAPES = {"slice": lambda c: (c[0],) + tuple(c[3:6]), "first": lambda c: (c[0],) + tuple(c[2:5]), "dense": None,
          "stats": lambda c: (c[0],) + tuple(c[3:6]), "cat": lambda c: (c[0],) + tuple(c[4]), "capi_stats": lambda c: (c[2],) + tuple(c[7]),
          "stats_fwd": lambda c: (c[0],) + tuple(c[3:6]), "geom": lambda c: (c[0],) + tuple(c[3]), "transpose": lambda c: (c[0],) + transpose_out(c),
          "ws_wgrad": lambda c: (c[2][0],) + tuple(c[2][3])}




# ================================================================== tests/test_fuzz_gpu.py
def _random_cases(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    chans = [8, 16, 24, 32, 48, 64]
    out = []
    for _ in range(n):
        ci, co = int(rng.choice(chans)), int(rng.choice(chans))
        d, h, w = int(rng.integers(1, 11)), int(rng.integers(1, 15)), int(rng.integers(1, 40))
        nb = int(rng.integers(1, 3))
        pad_in, pad_out = int(rng.choice([0, 8, 16])), int(rng.choice([0, 8]))
        out.append((nb, ci, co, d, h, w, pad_in, pad_out, int(rng.integers(0, 1 << 30))))
    return out


_LDS_FREE_SMALL = "direct nt1 mode0 split1"      # a workgroup per unit, its waves share the taps: fewer than 1024 units

# seeded random geometries, batch 1-2: bf16 on the tiled kernels (NT 1 / NT 2 / row-paired), fp32 too small for them
RANDOM = Table("RANDOM", "slice", _random_cases(14, 2024),
               {"f32": {"fwd": _LDS_FREE_SMALL, "dgrad": _LDS_FREE_SMALL}, "bf16": {"wgrad": "bf16"}})

# channel slices whose base address is NOT 16-byte aligned (pad_in = 2 fp32 elements / 2 or 4 bf16 elements, odd pitches):
# legal inputs that the MFMA kernels (16-byte pieces) cannot take — the dispatcher must fall back to the generic kernels
# instead of failing with EINVAL.  (pad_in = 4 fp32 elements IS 16-byte aligned: that case stays on the MFMA kernels in fp32; the
# incoming gradient starts its buffer, so the data gradient is generic only where its pitch is odd.)
MISALIGNED = Table("MISALIGNED", "slice", [(1, 16, 16, 5, 9, 20, 2, 0, 11), (2, 8, 16, 4, 8, 16, 2, 2, 12), (1, 48, 16, 3, 8, 17, 4, 4, 13),
                                           (1, 16, 32, 6, 10, 18, 6, 0, 14), (1, 32, 32, 2, 3, 5, 1, 3, 15)],
                   {"f32": {}, "bf16": {"fwd": "generic", "wgrad": "generic"}})

# fp32 volumes with fewer than MRI3D_SMALL_UNITS = 512 (tile, N-block) work units go to the LDS-free kernel; these ragged shapes (two
# ragged tiles per axis) have the batch for 512 units or more, so that the TILED fp32 kernel keeps its border tiles covered: NT 1 and
# NT 2, three N-blocks in the data gradient (48 channels), pitched inputs and gradients
TILED_F32 = Table("TILED_F32", "slice", [(64, 16, 16, 5, 9, 19, 0, 0, 21), (64, 32, 32, 5, 9, 17, 8, 8, 22), (64, 48, 16, 5, 9, 21, 0, 8, 23),
                                         (72, 8, 32, 5, 9, 17, 8, 0, 24)],
                  {"f32": {"fwd": "tiled"}}, dtypes=("f32",))

# the same ragged shapes with batches that stay under 512 units: the LDS-free kernel with a wave per M-tile (1024 units or more)
DIRECT_F32_BATCH = Table("DIRECT_F32_BATCH", "slice", [(40, 16, 16, 5, 9, 19, 0, 0, 21), (24, 8, 32, 6, 11, 17, 8, 0, 22), (48, 48, 16, 3, 7, 21, 0, 8, 23)],
                         {"f32": {"fwd": "direct nt1 mode0 split0", "dgrad": "direct nt1 mode0 split0"}}, dtypes=("f32",))

# deep-level shapes of Modified3DUNet (batch 1): served by the LDS-free kernel in fp32 (1 and 2 N-tiles per wave)
SMALL = Table("SMALL", "slice", [(1, 64, 64, 20, 24, 20, 0, 0, 31), (1, 128, 128, 10, 12, 10, 0, 0, 32), (1, 128, 64, 20, 24, 20, 0, 0, 33),
                                 (1, 32, 32, 40, 48, 40, 0, 0, 34), (2, 24, 48, 7, 5, 9, 8, 8, 35), (1, 16, 16, 3, 3, 3, 0, 0, 36)],
              {"f32": {"fwd": "direct", "dgrad": "direct"}}, dtypes=("f32",))

# the LDS-free kernel with 2 and 4 N-tiles per wave (4096 or more M-tiles per N-block), ragged: a volume under 512 tile units,
# and volumes at most 8 voxels wide, which take it whatever the batch
DIRECT_WIDE = Table("DIRECT_WIDE", "slice", [(1, 32, 32, 39, 47, 41, 0, 0, 101), (150, 16, 64, 7, 9, 7, 0, 0, 102), (150, 64, 16, 7, 9, 7, 8, 0, 103)],
                    {"f32": {"fwd": "direct", "dgrad": "direct"}}, dtypes=("f32",))

# many small volumes: 512 or more (tile, N-block) units keep fp32 on the tiled kernel (the first four forwards); ragged tile borders
# in every dimension, 1 / 2 / 3 chunks, three N-blocks (the 48-channel data gradient), pitched inputs and outputs; then
# volumes at most 8 voxels wide, which go to the LDS-free MFMA kernel in fp32 whatever the batch (two rows per 16-voxel M-tile; an
# M-tile may straddle rows, planes and samples): the patch CNN's 8^3 level, a ragged one, pitched, > 32 MB of input
LARGE_BATCH = Table("LARGE_BATCH", "slice", [(64, 16, 16, 9, 13, 21, 0, 0, 41), (72, 48, 16, 5, 9, 19, 0, 8, 42), (96, 16, 48, 3, 10, 17, 16, 0, 43),
                                             (40, 32, 16, 11, 9, 33, 8, 8, 44), (260, 16, 16, 2, 3, 5, 0, 0, 45),
                                             (128, 32, 64, 8, 8, 8, 0, 0, 46), (70, 16, 24, 5, 7, 6, 8, 0, 47), (300, 64, 64, 8, 8, 8, 0, 0, 48)],
                    {"f32": {"wgrad": "wgrad6"}, "bf16": {"fwd": "tiled"}})

# bf16 weight gradient marching along d (conv_mfma_wgrad_bf16t_kernel in conv_mfma_wgrad.hip, LDS-DMA rows + transposing reads: taken when columns x
# segments >= 3 tasks per workgroup): a last segment of 5 / 3 / 1 planes, a last row tile of one row, a last column tile of 5 voxels,
# an 8-channel input tile (upper half empty) read from a pitched buffer, 24 output channels (half-empty second block) written from
# a pitched gradient
MARCH_WGRAD = Table("MARCH_WGRAD", "slice", [(8, 64, 64, 45, 17, 37, 0, 0, 91), (24, 8, 128, 23, 9, 33, 8, 0, 92), (64, 32, 24, 41, 12, 20, 0, 8, 93)],
                    {"bf16": {"wgrad": "bf16t"}}, dtypes=("bf16",))

# exactly 8 output channels in the forward (8 -> 8, 16 -> 8, 24 -> 8) or in the data gradient (8 -> 16, 8 -> 32).  bf16: the row-paired
# variant of the tiled MFMA kernel (two taps share the 16-row weight operand, 9 accumulators, halves folded in the epilogue), ragged
# in every axis, pitched slices, one case with a single chunk.  fp32: under 512 work units, so the LDS-free kernel; the weight
# gradient with paired operand halves (wgrad6 ci8 / co8): 32 -> 8, pitched 8 -> 8, one-tile and W < 16 volumes.  (The fp32 row-paired
# kernel has its cases in N8_TILED.)
N8 = Table("N8", "slice", [(2, 8, 8, 21, 35, 50, 0, 0, 71), (1, 16, 8, 17, 40, 65, 8, 8, 72), (2, 24, 8, 9, 33, 47, 0, 0, 73),
                           (1, 8, 16, 13, 41, 70, 0, 8, 74), (1, 8, 32, 9, 34, 49, 8, 0, 75), (40, 8, 8, 4, 8, 16, 0, 0, 76),
                           (1, 32, 8, 11, 19, 37, 0, 0, 77), (1, 8, 8, 7, 13, 33, 8, 8, 78), (3, 8, 8, 2, 6, 16, 0, 0, 79), (2, 16, 8, 5, 7, 9, 0, 0, 80)],
           {"f32": {"fwd": "direct nt1 mode0", "dgrad": "direct nt1 mode0"}, "bf16": {"wgrad": "bf16"}})

# the row-paired tiled kernel in BOTH storage types: batch 64 of a 5x9x17 volume is 512 tile units (two ragged tiles per axis), so
# fp32 stays on the tiled kernels: 8 -> 8 (forward and data gradient), 16 -> 8 (forward), 8 -> 16 (data gradient), pitched variants
N8_TILED = Table("N8_TILED", "slice", [(64, 8, 8, 5, 9, 17, 0, 0, 81), (64, 16, 8, 5, 9, 17, 8, 8, 82), (64, 8, 16, 5, 9, 17, 0, 8, 83), (64, 8, 8, 5, 9, 17, 8, 8, 84)],
                 {"f32": {}, "bf16": {}})

# stride-2 3x3x3 layers (modified_3dunet.py:23-38, cnn_model.py:49-81) on the LDS-free MFMA kernel: forward over output M-tiles,
# data gradient over same-parity input M-tiles with wave-uniform tap sets; even / odd extents (the last output voxel then has no
# kw = 2 neighbour), pitched slices, few units (a workgroup per unit, taps split over its waves) and many, Kc = 8 (half a chunk)
STRIDED = Table("STRIDED", "slice", [(1, 8, 16, 16, 18, 20, 0, 0, 51), (1, 16, 32, 9, 11, 13, 0, 0, 52), (2, 32, 64, 10, 12, 9, 8, 16, 53),
                                     (1, 64, 128, 6, 7, 5, 0, 0, 54), (1, 8, 16, 40, 48, 40, 0, 0, 55), (3, 24, 40, 5, 6, 33, 0, 8, 56),
                                     (1, 16, 8, 7, 9, 37, 0, 0, 57), (1, 8, 16, 2, 3, 1, 0, 0, 58)],
                {"f32": {"fwd": _LDS_FREE_SMALL, "dgrad": "direct nt1 mode1"}, "bf16": {"fwd": _LDS_FREE_SMALL, "dgrad": "direct nt1 mode1", "wgrad": "bf16"}},
                stride=2)

# stride 2 with enough M-tiles for a wave per tile and for 2 / 4 N-tiles per wave: the data gradient from 4096 same-parity M-tiles
# per N-block (32 and 64 input channels), the forward from 1024 and from 4096 output M-tiles (32 and 64 output channels); all ragged
STRIDED_WIDE = Table("STRIDED_WIDE", "slice", [(4, 32, 16, 21, 25, 19, 0, 0, 111), (4, 64, 16, 21, 25, 19, 0, 8, 112), (2, 8, 16, 41, 41, 41, 0, 0, 113),
                                               (1, 8, 32, 81, 81, 81, 0, 0, 114), (1, 8, 64, 81, 81, 81, 0, 0, 115)],
                     {"f32": {"fwd": "direct", "dgrad": "direct"}, "bf16": {"fwd": "direct", "dgrad": "direct", "wgrad": "bf16"}}, stride=2)

STRIDE3 = Table("STRIDE3", "slice", [(1, 16, 32, 10, 11, 13, 0, 0, 61), (2, 8, 16, 7, 8, 19, 8, 0, 62)],
                {"f32": {"fwd": _LDS_FREE_SMALL, "dgrad": "direct nt1 mode1 split1", "wgrad": "generic"}}, dtypes=("f32",), stride=3)

# bf16 tensors the bf16 MFMA weight-gradient kernels cannot take (output channels or a gradient pitch that are no multiple of 8):
# wgrad4 with 16 | Cin (12 and 20 output channels, a gradient of pitch 20), wgrad3 with 8 | Cin; ragged, several tiles per axis
BF16_WGRAD_QUADS = Table("BF16_WGRAD_QUADS", "slice", [(2, 16, 12, 5, 13, 37, 0, 0, 121), (2, 16, 20, 5, 9, 17, 8, 0, 122), (2, 32, 12, 7, 13, 33, 0, 0, 123),
                                                       (2, 16, 16, 5, 13, 37, 0, 4, 124), (2, 8, 12, 5, 13, 37, 0, 0, 125), (2, 24, 20, 5, 9, 17, 0, 0, 126)],
                         {"bf16": {"dgrad": "generic"}}, dtypes=("bf16",))   # (12 / 20 gradient channels: no 16-byte pieces)

# the marching kernel where the DISPATCHER chooses it (bf16, one 16-channel output block, a grid of 192 workgroups or more): 48
# volumes with four 11-plane segments each, one and four columns per workgroup, pitched, three N-blocks in the data gradient
MARCH_BF16 = Table("MARCH_BF16", "slice", [(48, 16, 16, 41, 5, 9, 0, 0, 131), (48, 16, 16, 41, 9, 17, 0, 0, 132), (48, 32, 16, 41, 5, 9, 8, 8, 133),
                                           (48, 16, 48, 41, 5, 9, 0, 0, 134)],
                   {"bf16": {"dgrad": "march"}}, dtypes=("bf16",))
MARCH_BF16_NOBIAS = Table("MARCH_BF16_NOBIAS", "slice", [(48, 8, 16, 41, 5, 9, 0, 0, 141)], {"bf16": {"fwd": "march", "dgrad": "march"}},
                          dtypes=("bf16",), bias=False)

# The weight-gradient kernels reserve the dbias accumulator only in their BIAS instantiations, and the partial layout they share
# (TGA = tap groups + 1) changes with it: the bias-less twins of rows above that no other table reaches — the same small ragged
# geometries as in BF16_WGRAD_QUADS (8 -> 12, 16 -> 12), N8 (8 -> 8 pitched, 32 -> 8) and MARCH_WGRAD (8 -> 128 marching along d)
WGRAD_NOBIAS = Table("WGRAD_NOBIAS", "slice", [(2, 8, 12, 5, 13, 37, 0, 0, 151), (2, 16, 12, 5, 13, 37, 0, 0, 152), (1, 8, 8, 7, 13, 33, 8, 8, 153),
                                               (1, 32, 8, 11, 19, 37, 0, 0, 154), (24, 8, 128, 23, 9, 33, 8, 0, 155)],
                     {"f32": {"wgrad": ("wgrad3", "wgrad6", "wgrad6 ci8 co8", "wgrad6 co8", "wgrad3")},
                      "bf16": {"wgrad": ("wgrad3", "wgrad4", "bf16", "bf16", "bf16t")}}, bias=False)

# the forward with fused BatchNorm statistics against the CPU reference (y and the statistics): the tiled kernel with 1 and 2
# N-tiles per wave, the marching kernel with and without a bias (bf16; fp32 takes it from 4 Mi voxels up only)
STATS_ORACLE = Table("STATS_ORACLE", "stats_fwd", [(2, 16, 16, 5, 9, 17, True), (2, 8, 32, 5, 9, 17, False), (48, 16, 16, 41, 5, 9, True),
                                                   (48, 8, 16, 41, 5, 9, False)],
                     {"f32": {"stats": "tiled"}, "bf16": {}}, ids=lambda c: "n%d_%d-%d_%dx%dx%d_b%d" % c)

# Conv3d(1, 8|16, 3, padding=1): the direct first-layer kernels of conv_generic.hip (conv_cin1_{fwd,wgrad}_kernel); 16 output
# channels take the MFMA file's cin1 weight gradient
FIRST = Table("FIRST", "first", [(2, 8, 9, 13, 37, True, 0), (1, 16, 8, 16, 32, False, 0), (1, 8, 4, 8, 32, False, 8), (3, 16, 5, 7, 19, True, 0),
                                 (1, 8, 1, 1, 1, True, 0), (1, 8, 17, 9, 70, True, 8), (2, 16, 6, 20, 33, True, 16), (1, 8, 12, 24, 64, False, 0)],
              {"f32": {"fwd": "generic", "dgrad": "generic"}, "bf16": {"fwd": "generic", "dgrad": "generic"}},
              ids=lambda c: "n%d_1-%d_%dx%dx%d_b%d_p%d" % c)


class DenseTable(Table):
    """fields(case) -> (n, ci, co, (d, h, w), k, s, p, dil, bias); case_dtype(case) -> the one dtype of a case, where it has one."""

    def __init__(self, name, cases, expect, fields, case_dtype=None, **kw):
        self.fields, self.case_dtype = fields, case_dtype
        Table.__init__(self, name, "dense", cases, expect, **kw)

    def shape(self, case, pass_="fwd"):
        f = self.fields(case)
        return (f[0],) + tuple(f[3])


ONE_OUT = DenseTable("ONE_OUT", [(2, 8, (3, 1, 1), (1, 0, 0), (1, 1, 1), (9, 13, 37), True), (1, 1, (1, 3, 1), (0, 1, 0), (1, 1, 1), (4, 8, 32), False),
                                 (1, 1, (1, 1, 3), (0, 0, 1), (1, 1, 1), (5, 7, 19), True), (2, 4, (1, 6, 1), (0, 2, 0), (1, 2, 1), (6, 20, 9), True),
                                 (1, 16, (1, 1, 3), (0, 0, 1), (1, 1, 1), (3, 5, 70), False), (2, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), (9, 13, 37), True),
                                 (1, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True), (1, 8, (6, 1, 1), (2, 0, 0), (2, 1, 1), (12, 6, 10), True)],
                     {"f32": {"fwd": "generic", "dgrad": "generic", "wgrad": "generic"}},
                     fields=lambda c: (c[0], c[1], 1, c[5], c[2], c[4], c[3], 1, c[6]), dtypes=("f32",),
                     ids=lambda c: "n%d_%d-1_k%s_s%s_%s" % (c[0], c[1], "x".join(map(str, c[2])), "".join(map(str, c[4])), "x".join(map(str, c[5]))))

# ================================================================== tests/test_ops_gpu.py
OPS_CONV = DenseTable("OPS_CONV", [
    # name, N, Cin, Cout, (D,H,W), k, s, p, d, bias
    ("unet_1_8", 2, 1, 8, (12, 20, 16), 3, 1, 1, 1, True),
    ("unet_8_16", 2, 8, 16, (12, 20, 16), 3, 1, 1, 1, True),
    ("unet_16_16", 1, 16, 16, (16, 12, 20), 3, 1, 1, 1, True),
    ("unet_16_32", 1, 16, 32, (8, 12, 16), 3, 1, 1, 1, True),
    ("unet_32_32", 1, 32, 32, (8, 12, 8), 3, 1, 1, 1, True),
    ("unet_32_64", 1, 32, 64, (8, 6, 8), 3, 1, 1, 1, True),
    ("unet_96_32", 1, 96, 32, (8, 8, 12), 3, 1, 1, 1, True),
    ("unet_48_16", 1, 48, 16, (12, 16, 16), 3, 1, 1, 1, True),
    ("unet_cls_16_2", 2, 16, 2, (12, 20, 16), 1, 1, 0, 1, True),
    ("pw_32_2", 1, 32, 2, (9, 10, 11), 1, 1, 0, 1, False),
    ("pw_64_8", 2, 64, 8, (6, 7, 8), 1, 1, 0, 1, True),
    ("pw_16_5", 1, 16, 5, (6, 7, 8), 1, 1, 0, 1, True),
    ("pw_128_64", 1, 128, 64, (4, 5, 6), 1, 1, 0, 1, False),
    ("pw_8_3", 2, 8, 3, (5, 9, 13), 1, 1, 0, 1, True),       # forward on the lanes-per-voxel kernel: 2 / 1 / 16 lanes per voxel,
    ("pw_4_1", 1, 4, 1, (7, 6, 5), 1, 1, 0, 1, False),       # 1-4 output channels, voxel counts that are no multiple of anything
    ("pw_64_4", 1, 64, 4, (3, 7, 11), 1, 1, 0, 1, True),
    ("mfma_24_40", 1, 24, 40, (6, 9, 17), 3, 1, 1, 1, True),
    ("mfma_64_128_ragged", 1, 64, 128, (3, 5, 7), 3, 1, 1, 1, False),
    ("ragged_3x3x3", 1, 16, 16, (5, 7, 9), 3, 1, 1, 1, False),
    ("tiny_1voxel", 1, 8, 16, (1, 1, 1), 3, 1, 1, 1, True),
    ("sepx_k6s2p2", 2, 1, 8, (32, 12, 10), (6, 1, 1), (2, 1, 1), (2, 0, 0), 1, True),
    ("sepy_k6s2p2", 2, 8, 8, (8, 24, 10), (1, 6, 1), (1, 2, 1), (0, 2, 0), 1, True),
    ("sepz_k6s2p2", 2, 8, 16, (8, 6, 28), (1, 1, 6), (1, 1, 2), (0, 0, 2), 1, True),
    ("sepx_k3p0", 3, 32, 64, (3, 3, 3), (3, 1, 1), 1, 0, 1, True),
    ("sepz_k3p1", 1, 16, 8, (6, 5, 9), (1, 1, 3), 1, (0, 0, 1), 1, True),
    ("stride2_m3d", 1, 8, 16, (12, 10, 14), 3, 2, 1, 1, False),
    ("stride2_odd", 1, 16, 32, (9, 7, 11), 3, 2, 1, 1, False),
    ("dilated_s2", 1, 1, 4, (25, 23, 27), 3, 2, 0, 3, True),
    ("dilated_p3", 1, 4, 4, (11, 12, 13), 3, 1, 3, 3, True),
    ("reduce_k4s4", 1, 1, 1, (16, 12, 8), 4, 4, 0, 1, True),
    ("vox_1_1", 2, 1, 1, (9, 10, 11), 3, 1, 1, 1, True),
    # 1 -> 1 separable convs of the autoencoder's last block (AE_model.py:110-160): the 16-byte stencil kernels (W % 4 == 0) ...
    ("c1_sepy", 2, 1, 1, (9, 10, 12), (1, 3, 1), 1, (0, 1, 0), 1, True),
    ("c1_sepz", 2, 1, 1, (5, 7, 16), (1, 1, 3), 1, (0, 0, 1), 1, True),
    ("c1_sepx_nobias", 1, 1, 1, (6, 5, 8), (3, 1, 1), 1, (1, 0, 0), 1, False),
    ("c1_sepz_k6_p2", 1, 1, 1, (4, 6, 20), (1, 1, 6), 1, (0, 0, 2), 1, True),      # output narrower than the input (W 20 -> 19: gather path)
    ("c1_sepz_k5_p2_dil2", 1, 1, 1, (4, 6, 24), (1, 1, 5), 1, (0, 0, 4), 2, True),  # dilation 2, same width: shifted 16-byte loads
    ("c1_sepy_k2", 2, 1, 1, (4, 9, 8), (1, 2, 1), 1, (0, 1, 0), 1, True),           # even filter: H 9 -> 10
    # ... and a width that is not a multiple of 4 (gather kernels)
    ("c1_sepz_ragged", 1, 1, 1, (5, 6, 10), (1, 1, 3), 1, (0, 0, 1), 1, True),
    ("odd_channels", 1, 3, 5, (6, 7, 8), 3, 1, 1, 1, True),
    ("wide_128", 1, 128, 128, (4, 4, 4), 3, 1, 1, 1, False),
], {"f32": {}}, fields=lambda c: c[1:], dtypes=("f32",), ids=lambda c: c[0])

# conv3d(bn_stats=True) against conv3d + a statistics pass: ragged sizes (masked tile borders), one and two N-tiles per wave,
# several passes (Cout 48); the fused forward is always the tiled kernel here, the plain fp32 one mostly the LDS-free kernel
OPS_STATS = Table("OPS_STATS", "stats", [(2, 16, 16, 9, 13, 21, True), (1, 48, 16, 8, 16, 32, True), (2, 8, 32, 5, 8, 16, False),
                                         (1, 32, 64, 4, 9, 17, True), (1, 16, 48, 6, 7, 19, True),
                                         (64, 16, 16, 9, 13, 21, True), (90, 48, 16, 3, 9, 17, False), (88, 16, 48, 5, 7, 19, True)],
                  {"f32": {"stats": "tiled"}, "bf16": {"stats": "tiled", "fwd": "tiled", "wgrad": "bf16"}},
                  oracle=False, ids=lambda c: "n%d_%d-%d_%dx%dx%d_b%d" % c)

# (batch, Ca, Cb, Cout, volume, channel padding of the second tensor's buffer, bias, served by the split kernels in fp32 / bf16)
CAT = Table("CAT", "cat", [(2, 16, 32, 16, (24, 40, 70), 0, True, True, True), (2, 32, 64, 32, (21, 33, 70), 8, True, True, True),
                           (8, 32, 64, 32, (45, 17, 37), 8, True, True, True),       # bf16: the weight gradient marches along d (3 segments of 20)
                           (5, 16, 16, 8, (17, 40, 65), 0, False, True, True),       # (>= 512 work units in every pass: below that the plain convolution
                                                                                     #  prefers the LDS-free kernel and the sums are ordered differently)
                           (2, 16, 24, 16, (24, 40, 70), 0, True, False, True),      # 24 trailing channels: not a ci-tile multiple for the fp32 weight gradient
                           (1, 8, 16, 16, (24, 40, 70), 0, True, False, False),      # 8 leading channels: the split must be a multiple of 16
                           (1, 16, 32, 16, (6, 7, 9), 0, True, False, True),         # tiny volume: fp32 runs on the LDS-free kernel (no split support)
                           (5, 16, 16, 16, (17, 40, 65), 4, True, True, False)],     # second tensor of pitch 20: fp32 served (16-byte aligned slice),
                                                                                     # bf16 falls back (the slice starts 8 bytes into the voxel)
            {"f32": {}, "bf16": {}}, oracle=False,
            ids=lambda c: "n%d_%d+%d-%d_%s_p%d_b%d" % (c[0], c[1], c[2], c[3], "x".join(map(str, c[4])), c[5], c[6]))

# ================================================================== tests/test_bf16_gpu.py
BF16_CONV = DenseTable("BF16_CONV", [
    # (n, ci, co, size, k, stride, pad, dil)
    (2, 8, 16, (12, 20, 18), 3, 1, 1, 1),       # MFMA-shaped 3x3x3
    (1, 16, 16, (9, 17, 33), 3, 1, 1, 1),
    (1, 48, 16, (8, 16, 16), 3, 1, 1, 1),
    (2, 32, 64, (6, 9, 17), 3, 1, 1, 1),
    (1, 96, 32, (5, 8, 16), 3, 1, 1, 1),
    (2, 1, 8, (10, 12, 14), 3, 1, 1, 1),        # first layer
    (2, 16, 2, (10, 12, 14), 1, 1, 0, 1),       # classifier
    (1, 32, 2, (9, 10, 11), 1, 1, 0, 1),        # pointwise heads: 8 channels per lane, vector dy loads; ragged voxel counts
    (2, 64, 4, (5, 7, 9), 1, 1, 0, 1),
    (1, 16, 5, (6, 7, 8), 1, 1, 0, 1),
    (1, 24, 3, (6, 7, 8), 1, 1, 0, 1),
    (1, 8, 16, (11, 12, 13), 3, 2, 1, 1),       # strided (Modified3DUNet)
    (1, 4, 6, (9, 10, 11), (3, 1, 1), (2, 1, 1), (1, 0, 0), 1),
], {"bf16": {}}, fields=lambda c: c + (True,), dtypes=("bf16",),
    ids=lambda c: "n%d_%d-%d_%s_k%s_s%s" % (c[0], c[1], c[2], "x".join(map(str, c[3])), c[4], c[5]))

# ================================================================== tests/test_buffer_contracts_gpu.py
FULL = (160, 192, 160)      # the U-Net's full-resolution level: >= 4 M voxels, where the fp32 marching kernel is chosen
# patterns of launched kernel names (torch profiler), demangled or not
TILED_KERNEL = r"conv_mfma_fwd2_kernel"
N8_KERNEL = r"conv_mfma_fwd2_kernel(<.*, false, true>|I.*Lb0ELb1EE)"     # <T, NT, stats = false, n8 = true>
MARCH_KERNEL = r"conv_march_kernel"
DIRECT_KERNEL = r"conv_mfma_direct_kernel"

# (id, dtype, n, ca, cb, second-tensor pitch, co, volume, kernel the dispatcher must pick)
CAPI_STATS = Table("CAPI_STATS", "capi_stats", [
    ("f32_tiled", "f32", 2, 16, 0, 0, 32, (19, 37, 70), TILED_KERNEL),
    ("bf16_tiled", "bf16", 2, 16, 0, 0, 32, (19, 37, 70), TILED_KERNEL),       # 32 output channels: two blocks, never the marching kernel
    ("f32_march", "f32", 1, 16, 0, 0, 16, FULL, MARCH_KERNEL),
    ("bf16_march", "bf16", 1, 16, 0, 0, 16, FULL, MARCH_KERNEL),
    ("f32_cat_tiled", "f32", 2, 16, 16, 16, 16, (24, 40, 70), TILED_KERNEL),
    ("bf16_cat_tiled", "bf16", 2, 16, 16, 16, 32, (24, 40, 70), TILED_KERNEL),
    ("f32_cat_march", "f32", 1, 16, 16, 16, 16, FULL, MARCH_KERNEL),
    ("bf16_cat_march", "bf16", 1, 16, 16, 16, 16, FULL, MARCH_KERNEL),
    # the split-operand overrun: a second tensor of pitch 20 / 28 (fp32, served) runs the tiled kernel (512 blocks) where the
    # one-tensor query answers with the marching kernel's grid
    ("f32_cat_ld20", "f32", 1, 16, 16, 20, 16, FULL, TILED_KERNEL),
    ("f32_cat_ld28", "f32", 1, 16, 16, 28, 16, FULL, TILED_KERNEL),
], {"f32": {}, "bf16": {}}, oracle=False, ids=lambda c: c[0])      # (a float64 reference at sampled voxels, computed on the device)
CAPI_STATS.case_dtype = lambda c: c[1]

# (id, dtype, n, ci, co, volume, k, pad, dil, seed, kernel that must be among the launched ones) of the exact-workspace test
WS_CONV = DenseTable("WS_CONV", [
    ("conv_generic_odd_dilated", "f32", 1, 3, 5, (9, 10, 11), 3, 2, 2, 30, r"conv_fwd_(generic|taps)_kernel"),
    ("conv_pointwise", "f32", 2, 32, 2, (9, 10, 11), 1, 0, 1, 31, r"pw_fwd_kernel"),
    ("conv_small_f32", "f32", 1, 32, 32, (10, 12, 10), 3, 1, 1, 32, DIRECT_KERNEL),
    ("conv_narrow_f32", "f32", 64, 16, 16, (8, 8, 8), 3, 1, 1, 33, DIRECT_KERNEL),
    ("conv_tiled_f32", "f32", 5, 16, 16, (17, 40, 65), 3, 1, 1, 34, TILED_KERNEL),   # >= 512 work units
    ("conv_tiled_bf16", "bf16", 2, 16, 32, (19, 37, 70), 3, 1, 1, 35, TILED_KERNEL),
    ("conv_n8_bf16", "bf16", 1, 16, 8, (17, 40, 65), 3, 1, 1, 36, N8_KERNEL),
    ("conv_march_f32", "f32", 1, 16, 16, FULL, 3, 1, 1, 37, MARCH_KERNEL),
    ("conv_march_bf16", "bf16", 1, 16, 16, FULL, 3, 1, 1, 38, MARCH_KERNEL),
    ("conv_wgrad_bf16_march_d", "bf16", 8, 64, 64, (45, 17, 37), 3, 1, 1, 39, r"conv_mfma_wgrad_bf16t_kernel"),
], {"f32": {}, "bf16": {}}, fields=lambda c: (c[2], c[3], c[4], c[5], c[6], 1, c[7], c[8], True), case_dtype=lambda c: c[1], oracle=False,
    ids=lambda c: c[0])


# ================================================================== tests/test_conv_variants_gpu.py
# Every kernel and instantiation of conv_generic.hip and conv_pointwise.hip (the route names "generic ..." / "pointwise ..."), in fp32
# and bf16.  The case lists are a greedy cover of tests/test_conv_routes.py's MATRIX over small volumes that are ragged in d, h and w
# (W a multiple of 4 with odd d and h for the 1 -> 1 taps kernels, which need it): separable filters of 2-6 taps along each axis with
# stride 1 and 2, 2x2x2, 1x2x2 (four taps), 3x3x1 / stride 2 (four valid taps in the data gradient), k4s4, k4s2, 3x3x3 with stride 2,
# one-axis strides, dilation 2 and 3, 5x5x5 and 1x1x1 on 1-72 channels, W of 33 and 65 for the slab-walk kernels; then by hand an
# extent of 1 per axis and W = 70.  PER_CASE pins every case to its three kernels.
def _geom_id(c):
    j = lambda t: "".join(map(str, t))
    return "n%d_%d-%d_%s_k%s_s%s_p%s_d%s_b%d_i%d_o%d" % (c[0], c[1], c[2], "x".join(map(str, c[3])), j(c[4]), j(c[5]), j(c[6]), j(c[7]), c[8], c[9], c[10])


def _transpose_id(c):
    j = lambda t: "".join(map(str, t))
    return "n%d_%d-%d_%s_k%s_s%s_p%s_o%s_b%d" % (c[0], c[1], c[2], "x".join(map(str, c[3])), j(c[4]), j(c[5]), j(c[6]), j(c[7]), c[8])


GENERIC_DENSE_CASES = [
    (1, 1, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0), (1, 1, 2, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 1, 3, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0), (1, 1, 4, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 1, 5, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 0, 0), (1, 1, 16, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 1, 72, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0), (1, 2, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 2, 3, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0), (1, 2, 5, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 2, 16, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 0, 0), (1, 3, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 3, 2, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0), (1, 3, 4, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 4, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0), (1, 4, 3, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 4, 4, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0), (1, 4, 5, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 4, 16, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0), (1, 5, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 5, 2, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0), (1, 5, 4, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 8, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 0, 0), (1, 16, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 16, 2, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 0, 0), (1, 16, 4, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 1, 1, (5, 7, 8), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 0, 0), (1, 1, 1, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 1, 4, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 3, 1, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 3, 4, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 5, 1, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 5, 4, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), False, 0, 0), (1, 16, 1, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 16, 4, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 1, 1, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 1, 3, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0), (1, 1, 4, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 1, 5, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), False, 0, 0), (1, 1, 16, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 3, 1, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0), (1, 3, 4, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 4, 1, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0), (1, 4, 3, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 4, 5, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), False, 0, 0), (1, 4, 16, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 5, 1, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), False, 0, 0), (1, 5, 4, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 16, 1, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0), (1, 16, 4, (5, 7, 9), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 1, 1, (5, 7, 8), (4, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0), (1, 1, 4, (5, 7, 9), (5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 3, 4, (5, 7, 9), (5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0), (1, 4, 1, (5, 7, 9), (5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 4, 3, (5, 7, 9), (5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0), (1, 4, 4, (5, 7, 9), (5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 4, 5, (5, 7, 9), (5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), False, 0, 0), (1, 4, 16, (5, 7, 9), (5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 5, 4, (5, 7, 9), (5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), False, 0, 0), (1, 16, 4, (5, 7, 9), (5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 1, 1, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 1, 3, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 1, 4, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 1, 5, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 1, 16, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 3, 4, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 4, 1, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 4, 3, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 4, 4, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 4, 5, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 4, 16, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 5, 4, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 16, 4, (5, 7, 9), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 1, 4, (5, 7, 9), (3, 3, 1), (2, 2, 1), (1, 1, 0), (1, 1, 1), True, 0, 0),
    (1, 3, 4, (5, 7, 9), (3, 3, 1), (2, 2, 1), (1, 1, 0), (1, 1, 1), True, 0, 0), (1, 4, 1, (5, 7, 9), (3, 3, 1), (2, 2, 1), (1, 1, 0), (1, 1, 1), True, 0, 0),
    (1, 4, 3, (5, 7, 9), (3, 3, 1), (2, 2, 1), (1, 1, 0), (1, 1, 1), True, 0, 0), (1, 4, 5, (5, 7, 9), (3, 3, 1), (2, 2, 1), (1, 1, 0), (1, 1, 1), False, 0, 0),
    (1, 4, 16, (5, 7, 9), (3, 3, 1), (2, 2, 1), (1, 1, 0), (1, 1, 1), True, 0, 0), (1, 5, 4, (5, 7, 9), (3, 3, 1), (2, 2, 1), (1, 1, 0), (1, 1, 1), False, 0, 0),
    (1, 16, 4, (5, 7, 9), (3, 3, 1), (2, 2, 1), (1, 1, 0), (1, 1, 1), True, 0, 0), (1, 1, 4, (5, 7, 9), (4, 4, 4), (2, 2, 2), (1, 1, 1), (1, 1, 1), True, 0, 0),
    (1, 3, 4, (5, 7, 9), (4, 4, 4), (2, 2, 2), (1, 1, 1), (1, 1, 1), True, 0, 0), (1, 5, 4, (5, 7, 9), (4, 4, 4), (2, 2, 2), (1, 1, 1), (1, 1, 1), False, 0, 0),
    (1, 16, 4, (5, 7, 9), (4, 4, 4), (2, 2, 2), (1, 1, 1), (1, 1, 1), True, 0, 0), (1, 1, 1, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 0, 0),
    (1, 1, 4, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 0, 0), (1, 1, 8, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), False, 0, 0),
    (1, 1, 16, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 0, 0), (1, 3, 4, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 0, 0),
    (1, 5, 4, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), False, 0, 0), (1, 16, 4, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 0, 0),
    (1, 1, 4, (5, 7, 9), (3, 3, 3), (2, 1, 1), (1, 1, 1), (1, 1, 1), True, 0, 0), (1, 3, 4, (5, 7, 9), (3, 3, 3), (2, 1, 1), (1, 1, 1), (1, 1, 1), True, 0, 0),
    (1, 5, 4, (5, 7, 9), (3, 3, 3), (2, 1, 1), (1, 1, 1), (1, 1, 1), False, 0, 0), (1, 16, 4, (5, 7, 9), (3, 3, 3), (2, 1, 1), (1, 1, 1), (1, 1, 1), True, 0, 0),
    (1, 4, 1, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 4, 2, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 4, 3, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 4, 4, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 4, 5, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), False, 0, 0), (1, 4, 8, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 8, 1, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), False, 0, 0), (1, 8, 2, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0),
    (1, 8, 3, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 0, 0), (1, 8, 4, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), False, 0, 0),
    (1, 8, 8, (1, 7, 9), (1, 3, 1), (1, 1, 1), (0, 1, 0), (1, 1, 1), True, 0, 0), (2, 16, 8, (3, 5, 70), (1, 1, 6), (1, 1, 2), (0, 0, 2), (1, 1, 1), True, 0, 0),
    (1, 1, 1, (5, 1, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 0, 0), (3, 4, 4, (5, 7, 1), (2, 2, 2), (1, 1, 1), (1, 1, 1), (1, 1, 1), False, 0, 0),
    (1, 8, 16, (9, 1, 33), (6, 1, 1), (2, 1, 1), (2, 0, 0), (1, 1, 1), True, 0, 0),
]
GENERIC_PITCHED_CASES = [
    (1, 1, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 4, 4), (1, 1, 2, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 4, 4),
    (1, 1, 4, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 4, 4), (1, 1, 72, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 4, 4),
    (1, 2, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 4, 4), (1, 1, 1, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), True, 4, 4),
    (1, 1, 4, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), True, 4, 4), (1, 1, 1, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 4, 4),
    (1, 1, 8, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), False, 4, 4), (1, 1, 16, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 4, 4),
    (1, 4, 1, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 4, 4), (1, 1, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 1, 1),
    (1, 1, 2, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 1, 1), (1, 1, 72, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), True, 1, 1),
    (1, 2, 1, (5, 7, 9), (2, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1), False, 1, 1), (1, 1, 1, (5, 7, 9), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), True, 1, 1),
    (1, 1, 1, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 1, 1), (1, 1, 8, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), False, 1, 1),
    (1, 4, 1, (5, 7, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 1, 1), (1, 1, 16, (5, 7, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 1, 0),
    (1, 8, 8, (5, 7, 70), (1, 1, 3), (1, 1, 1), (0, 0, 1), (1, 1, 1), True, 4, 4), (2, 1, 8, (1, 9, 13), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), True, 0, 4),
    (1, 16, 2, (3, 1, 11), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), True, 4, 0),
]
TRANSPOSE_CASES = [
    (1, 1, 1, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 1, 3, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 1, 5, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 1, 16, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 2, 1, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 2, 3, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 2, 5, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 2, 16, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 4, 1, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 4, 3, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 4, 5, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 4, 16, (2, 3, 17), (2, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (2, 1, 1, (3, 5, 7), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 0, 0), True), (2, 1, 3, (3, 5, 7), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 0, 0), True),
    (2, 1, 5, (3, 5, 7), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 0, 0), True), (2, 1, 16, (3, 5, 7), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 0, 0), True),
    (2, 4, 1, (3, 5, 7), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 0, 0), True), (2, 4, 3, (3, 5, 7), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 0, 0), True),
    (2, 4, 5, (3, 5, 7), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 0, 0), True), (2, 4, 16, (3, 5, 7), (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 0, 0), True),
    (1, 1, 1, (5, 7, 8), (3, 1, 1), (1, 1, 1), (1, 0, 0), (0, 0, 0), True), (1, 1, 1, (2, 3, 17), (4, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 1, 3, (2, 3, 17), (4, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 1, 5, (2, 3, 17), (4, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 1, 16, (2, 3, 17), (4, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 4, 1, (2, 3, 17), (4, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 4, 3, (2, 3, 17), (4, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 4, 5, (2, 3, 17), (4, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 4, 16, (2, 3, 17), (4, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (2, 4, 1, (3, 5, 7), (5, 1, 1), (1, 1, 1), (2, 0, 0), (0, 0, 0), True),
    (2, 4, 3, (3, 5, 7), (5, 1, 1), (1, 1, 1), (2, 0, 0), (0, 0, 0), True), (2, 4, 5, (3, 5, 7), (5, 1, 1), (1, 1, 1), (2, 0, 0), (0, 0, 0), True),
    (2, 4, 16, (3, 5, 7), (5, 1, 1), (1, 1, 1), (2, 0, 0), (0, 0, 0), True), (1, 1, 1, (5, 7, 8), (5, 1, 1), (1, 1, 1), (2, 0, 0), (0, 0, 0), True),
    (2, 1, 1, (3, 5, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1), (0, 0, 0), True), (2, 4, 1, (3, 5, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1), (0, 0, 0), True),
    (2, 4, 3, (3, 5, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1), (0, 0, 0), True), (2, 4, 5, (3, 5, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1), (0, 0, 0), True),
    (2, 4, 16, (3, 5, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1), (0, 0, 0), True), (1, 4, 1, (4, 6, 8), (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 4, 3, (4, 6, 8), (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 4, 5, (4, 6, 8), (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 4, 16, (4, 6, 8), (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (1, 4, 1, (3, 4, 5), (3, 3, 1), (2, 2, 1), (1, 1, 0), (0, 0, 0), True),
    (1, 4, 3, (3, 4, 5), (3, 3, 1), (2, 2, 1), (1, 1, 0), (0, 0, 0), True), (1, 4, 5, (3, 4, 5), (3, 3, 1), (2, 2, 1), (1, 1, 0), (0, 0, 0), True),
    (1, 4, 16, (3, 4, 5), (3, 3, 1), (2, 2, 1), (1, 1, 0), (0, 0, 0), True), (1, 4, 1, (4, 6, 8), (3, 3, 3), (2, 2, 2), (1, 1, 1), (0, 0, 0), True),
    (1, 4, 3, (4, 6, 8), (3, 3, 3), (2, 2, 2), (1, 1, 1), (0, 0, 0), True), (1, 4, 5, (4, 6, 8), (3, 3, 3), (2, 2, 2), (1, 1, 1), (0, 0, 0), True),
    (1, 4, 16, (4, 6, 8), (3, 3, 3), (2, 2, 2), (1, 1, 1), (0, 0, 0), True), (1, 4, 1, (4, 6, 8), (5, 5, 5), (2, 2, 2), (2, 2, 2), (0, 0, 0), True),
    (1, 4, 3, (4, 6, 8), (5, 5, 5), (2, 2, 2), (2, 2, 2), (0, 0, 0), True), (1, 4, 5, (4, 6, 8), (5, 5, 5), (2, 2, 2), (2, 2, 2), (0, 0, 0), True),
    (1, 4, 16, (4, 6, 8), (5, 5, 5), (2, 2, 2), (2, 2, 2), (0, 0, 0), True), (2, 1, 4, (3, 5, 7), (1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (2, 3, 4, (3, 5, 7), (1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True), (2, 5, 4, (3, 5, 7), (1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), True),
    (1, 6, 6, (5, 6, 7), (2, 2, 2), (2, 2, 2), (0, 0, 0), (0, 0, 0), True), (2, 1, 1, (3, 4, 5), (4, 4, 4), (4, 4, 4), (0, 0, 0), (0, 0, 0), True),
    (1, 8, 4, (5, 5, 6), (4, 4, 4), (2, 2, 2), (1, 1, 1), (0, 0, 0), True), (1, 4, 8, (4, 5, 3), (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), True),
    (1, 8, 8, (3, 4, 5), (4, 4, 4), (4, 4, 4), (0, 0, 0), (0, 0, 0), True), (1, 16, 16, (2, 3, 5), (4, 4, 4), (4, 4, 4), (0, 0, 0), (0, 0, 0), True),
    (1, 1, 1, (3, 5, 7), (4, 4, 4), (4, 4, 4), (0, 0, 0), (0, 0, 0), True), (2, 8, 8, (3, 5, 7), (4, 4, 4), (2, 2, 2), (1, 1, 1), (0, 0, 0), True),
    (2, 4, 8, (3, 5, 7), (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), True), (1, 8, 8, (1, 5, 7), (2, 2, 2), (2, 2, 2), (0, 0, 0), (0, 0, 0), False),
]

# dense tensors
GENERIC_DENSE = Table("GENERIC_DENSE", "geom", GENERIC_DENSE_CASES, {"f32": {}, "bf16": {}}, ids=_geom_id)
# pitched channel slices: pads of 4 (fp32: the slice stays 16-byte aligned and keeps its vector loads; bf16: 8 bytes), 1 (neither
# alignment nor a pitch that is a multiple of 4) and 2 (fp32: 8 bytes), on one side or both — at least one per kernel family and pass
# wherever the family's precondition allows the pitch
GENERIC_PITCHED = Table("GENERIC_PITCHED", "geom", GENERIC_PITCHED_CASES, {"f32": {}, "bf16": {}}, ids=_geom_id)
# ConvTranspose3d: the only way to the data gradient WITH a bias of every generic and pointwise data-gradient kernel; then the four
# cases of test_ops_gpu's test_conv_transpose3d, the shipped layers (AE_model.py:71: k = s = 4 on 8 -> 8 and 16 -> 16; :128: 1 -> 1
# k4 s4), k4 s2 p1, output_padding on odd extents, an extent of 1 without a bias
TRANSPOSE = Table("TRANSPOSE", "transpose", TRANSPOSE_CASES, {"f32": {}, "bf16": {}}, ids=_transpose_id)

# one exact-workspace case per weight-gradient family of conv_generic.hip / conv_pointwise.hip: every family lays its partials out
# differently.  In conv_generic.hip the plan (generic_wgrad_plan) owns that layout — part_floats, bias_floats, channel pitches — and
# both the launch's carve and conv_generic_workspace_bytes read it; these cases check the plan against what the kernels really
# write, with guard bands around a workspace of exactly the queried size.  The launched-kernel pattern doubles as the
# check that a route name means the kernel it says.  quads_dy_misaligned: an 8 -> 8 (1,3,1) layer is the channel-quad kernel's by
# geometry (gradient pitch 12), but its gradient starts 8 bytes into the voxel, so the launch falls through to `small`
_1, _0 = (1, 1, 1), (0, 0, 0)
WS_WGRAD = Table("WS_WGRAD", "ws_wgrad", [
    ("wgrad_c1c1", "f32", (2, 1, 1, (5, 7, 9), (3, 3, 3), _1, _1, _1, True, 0, 0), 0, 50, r"conv_c1c1_wgrad_kernel"),
    ("wgrad_c1taps", "f32", (2, 1, 1, (5, 7, 12), (1, 1, 3), _1, (0, 0, 1), _1, True, 0, 0), 0, 51, r"conv_c1_taps_wgrad_kernel"),
    ("wgrad_cin1", "f32", (2, 1, 8, (5, 7, 9), (3, 3, 3), _1, _1, _1, True, 0, 0), 0, 52, r"conv_cin1_wgrad_kernel"),
    ("wgrad_cin1_bf16", "bf16", (1, 1, 16, (5, 7, 9), (3, 3, 3), _1, _1, _1, True, 0, 4), 4, 53, r"conv_cin1_wgrad_kernel"),
    ("wgrad_co1", "f32", (2, 8, 1, (5, 7, 9), (3, 1, 1), _1, (1, 0, 0), _1, True, 0, 0), 0, 54, r"conv_wgrad_co1_kernel"),
    ("wgrad_quads", "f32", (2, 8, 8, (5, 7, 9), (1, 3, 1), _1, (0, 1, 0), _1, True, 0, 0), 0, 55, r"conv_wgrad_quads_kernel"),
    ("wgrad_quads_bf16", "bf16", (2, 8, 16, (5, 7, 33), (1, 1, 6), (1, 1, 2), (0, 0, 2), _1, True, 4, 0), 0, 56, r"conv_wgrad_quads_kernel"),
    ("wgrad_quads_dy_misaligned", "f32", (2, 8, 8, (5, 7, 9), (1, 3, 1), _1, (0, 1, 0), _1, True, 0, 4), 2, 57, r"conv_wgrad_small_kernel"),
    ("wgrad_small", "f32", (2, 3, 5, (5, 7, 9), (1, 1, 3), _1, (0, 0, 1), _1, True, 0, 0), 0, 58, r"conv_wgrad_small_kernel"),
    ("wgrad_lds", "f32", (1, 3, 5, (7, 9, 11), (3, 3, 3), _1, (2, 2, 2), (2, 2, 2), True, 1, 0), 0, 59, r"conv_wgrad_generic_kernel"),
    ("wgrad_pointwise", "f32", (2, 16, 2, (5, 7, 9), _1, _1, _0, _1, True, 0, 0), 0, 60, r"pw_wgrad_kernel"),
    ("wgrad_pointwise_bf16", "bf16", (2, 32, 4, (5, 7, 9), _1, _1, _0, _1, True, 0, 0), 0, 61, r"pw_wgrad_kernel"),
], {"f32": {"wgrad": ("generic c1c1", "generic c1taps nt3", "generic cin1 co8", "generic co1 ci8", "generic quads nt4 civ4", "generic small",
                      "generic small", "generic lds", "pointwise co2 vx4 dv1")},
    "bf16": {"wgrad": ("generic cin1 co16", "generic quads nt6 civ4", "pointwise co4 vx8 dv1")}}, oracle=False, ids=lambda c: c[0])
WS_WGRAD.case_dtype = lambda c: c[1]


def pairs(table):
    """(case, dtype) of everything the table's test runs."""
    cd = getattr(table, "case_dtype", None)
    return [(c, dt) for c in table.cases for dt in table.dtypes if cd is None or cd(c) == dt]


def all_pairs():
    return [(t, c, dt) for t in TABLES.values() for c, dt in pairs(t)]


# ================================================================== the route of every case, by name
# One row per case: the exact answer of the route query, in the order ORDER[kind] of its table.  A dispatcher change that moves a
# case shows up here row by row; update a row only together with the table's comment, and never below what `expect` declares.
PER_CASE.update({
    ("RANDOM", "f32"): {
        'n1_16-48_1x4x13_p16_8': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n1_64-8_2x13x4_p0_8': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 co8",
        'n2_16-16_5x9x32_p16_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n1_32-48_1x3x19_p16_8': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n1_32-32_4x5x6_p16_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n1_16-48_9x12x9_p0_8': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n1_24-16_1x4x6_p16_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad3",
        'n1_16-24_9x9x12_p16_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n2_24-24_5x14x10_p0_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad3",
        'n2_16-32_2x3x36_p8_8': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n2_8-64_1x5x18_p0_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad3",
        'n2_8-16_7x8x14_p8_8': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad3",
        'n1_48-16_6x8x36_p0_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n2_16-64_6x7x23_p8_8': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
    },
    ("RANDOM", "bf16"): {
        'n1_16-48_1x4x13_p16_8': "tiled nt1 | tiled nt1 | bf16",
        'n1_64-8_2x13x4_p0_8': "tiled_n8 | tiled nt2 | bf16",
        'n2_16-16_5x9x32_p16_0': "tiled nt1 | tiled nt1 | bf16",
        'n1_32-48_1x3x19_p16_8': "tiled nt1 | tiled nt2 | bf16",
        'n1_32-32_4x5x6_p16_0': "tiled nt2 | tiled nt2 | bf16",
        'n1_16-48_9x12x9_p0_8': "tiled nt1 | tiled nt1 | bf16",
        'n1_24-16_1x4x6_p16_0': "tiled nt1 | tiled nt2 | bf16",
        'n1_16-24_9x9x12_p16_0': "tiled nt2 | tiled nt1 | bf16",
        'n2_24-24_5x14x10_p0_0': "tiled nt2 | tiled nt2 | bf16",
        'n2_16-32_2x3x36_p8_8': "tiled nt2 | tiled nt1 | bf16",
        'n2_8-64_1x5x18_p0_0': "tiled nt2 | tiled_n8 | bf16",
        'n2_8-16_7x8x14_p8_8': "tiled nt1 | tiled_n8 | bf16",
        'n1_48-16_6x8x36_p0_0': "tiled nt1 | tiled nt1 | bf16",
        'n2_16-64_6x7x23_p8_8': "tiled nt2 | tiled nt1 | bf16",
    },
    ("MISALIGNED", "f32"): {
        'n1_16-16_5x9x20_p2_0': "generic gather tl16 vec0 | direct nt1 mode0 split1 | generic lds",
        'n2_8-16_4x8x16_p2_2': "generic gather tl16 vec0 | generic gather tl8 vec0 | generic lds",
        'n1_48-16_3x8x17_p4_4': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n1_16-32_6x10x18_p6_0': "generic gather tl16 vec0 | direct nt1 mode0 split1 | generic lds",
        'n1_32-32_2x3x5_p1_3': "generic gather tl16 vec0 | generic gather tl16 vec0 | generic lds",
    },
    ("MISALIGNED", "bf16"): {
        'n1_16-16_5x9x20_p2_0': "generic gather tl16 vec0 | tiled nt1 | generic lds",
        'n2_8-16_4x8x16_p2_2': "generic gather tl16 vec0 | generic gather tl8 vec0 | generic lds",
        'n1_48-16_3x8x17_p4_4': "generic gather tl16 vec1 | generic gather tl16 vec1 | generic lds",
        'n1_16-32_6x10x18_p6_0': "generic gather tl16 vec0 | tiled nt1 | generic lds",
        'n1_32-32_2x3x5_p1_3': "generic gather tl16 vec0 | generic gather tl16 vec0 | generic lds",
    },
    ("TILED_F32", "f32"): {
        'n64_16-16_5x9x19_p0_0': "tiled nt1 | tiled nt1 | wgrad6",
        'n64_32-32_5x9x17_p8_8': "tiled nt2 | tiled nt2 | wgrad6",
        'n64_48-16_5x9x21_p0_8': "tiled nt1 | tiled nt1 | wgrad6",
        'n72_8-32_5x9x17_p8_0': "tiled nt2 | tiled_n8 | wgrad3",
    },
    ("DIRECT_F32_BATCH", "f32"): {
        'n40_16-16_5x9x19_p0_0': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad6",
        'n24_8-32_6x11x17_p8_0': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad3",
        'n48_48-16_3x7x21_p0_8': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad6",
    },
    ("SMALL", "f32"): {
        'n1_64-64_20x24x20_p0_0': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad6",
        'n1_128-128_10x12x10_p0_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n1_128-64_20x24x20_p0_0': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad6",
        'n1_32-32_40x48x40_p0_0': "direct nt2 mode0 split0 | direct nt2 mode0 split0 | wgrad6",
        'n2_24-48_7x5x9_p8_8': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad3",
        'n1_16-16_3x3x3_p0_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
    },
    ("DIRECT_WIDE", "f32"): {
        'n1_32-32_39x47x41_p0_0': "direct nt2 mode0 split0 | direct nt2 mode0 split0 | wgrad6",
        'n150_16-64_7x9x7_p0_0': "direct nt4 mode0 split0 | direct nt1 mode0 split0 | wgrad6",
        'n150_64-16_7x9x7_p8_0': "direct nt1 mode0 split0 | direct nt4 mode0 split0 | wgrad6",
    },
    ("LARGE_BATCH", "f32"): {
        'n64_16-16_9x13x21_p0_0': "tiled nt1 | tiled nt1 | wgrad6",
        'n72_48-16_5x9x19_p0_8': "tiled nt1 | tiled nt1 | wgrad6",
        'n96_16-48_3x10x17_p16_0': "tiled nt1 | direct nt1 mode0 split0 | wgrad6",
        'n40_32-16_11x9x33_p8_8': "tiled nt1 | tiled nt2 | wgrad6",
        'n260_16-16_2x3x5_p0_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'n128_32-64_8x8x8_p0_0': "direct nt4 mode0 split0 | direct nt2 mode0 split0 | wgrad6",
        'n70_16-24_5x7x6_p8_0': "direct nt1 mode0 split0 | direct nt1 mode0 split1 | wgrad6",
        'n300_64-64_8x8x8_p0_0': "direct nt4 mode0 split0 | direct nt4 mode0 split0 | wgrad6",
    },
    ("LARGE_BATCH", "bf16"): {
        'n64_16-16_9x13x21_p0_0': "tiled nt1 | tiled nt1 | bf16",
        'n72_48-16_5x9x19_p0_8': "tiled nt1 | tiled nt1 | bf16",
        'n96_16-48_3x10x17_p16_0': "tiled nt1 | tiled nt1 | bf16",
        'n40_32-16_11x9x33_p8_8': "tiled nt1 | tiled nt2 | bf16",
        'n260_16-16_2x3x5_p0_0': "tiled nt1 | tiled nt1 | bf16",
        'n128_32-64_8x8x8_p0_0': "tiled nt2 | march | bf16",
        'n70_16-24_5x7x6_p8_0': "tiled nt2 | tiled nt1 | bf16",
        'n300_64-64_8x8x8_p0_0': "tiled nt2 | tiled nt2 | bf16t",
    },
    ("MARCH_WGRAD", "bf16"): {
        'n8_64-64_45x17x37_p0_0': "tiled nt2 | tiled nt2 | bf16t",
        'n24_8-128_23x9x33_p8_0': "tiled nt2 | tiled_n8 | bf16t",
        'n64_32-24_41x12x20_p0_8': "tiled nt2 | march | bf16t",
    },
    ("N8", "f32"): {
        'n2_8-8_21x35x50_p0_0': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad6 ci8 co8",
        'n1_16-8_17x40x65_p8_8': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad6 co8",
        'n2_24-8_9x33x47_p0_0': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad3",
        'n1_8-16_13x41x70_p0_8': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad3",
        'n1_8-32_9x34x49_p8_0': "direct nt1 mode0 split0 | direct nt1 mode0 split1 | wgrad3",
        'n40_8-8_4x8x16_p0_0': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad6 ci8 co8",
        'n1_32-8_11x19x37_p0_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 co8",
        'n1_8-8_7x13x33_p8_8': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 ci8 co8",
        'n3_8-8_2x6x16_p0_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 ci8 co8",
        'n2_16-8_5x7x9_p0_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 co8",
    },
    ("N8", "bf16"): {
        'n2_8-8_21x35x50_p0_0': "tiled_n8 | tiled_n8 | bf16",
        'n1_16-8_17x40x65_p8_8': "tiled_n8 | tiled nt1 | bf16",
        'n2_24-8_9x33x47_p0_0': "tiled_n8 | tiled nt2 | bf16",
        'n1_8-16_13x41x70_p0_8': "tiled nt1 | tiled_n8 | bf16",
        'n1_8-32_9x34x49_p8_0': "tiled nt2 | tiled_n8 | bf16",
        'n40_8-8_4x8x16_p0_0': "tiled_n8 | tiled_n8 | bf16",
        'n1_32-8_11x19x37_p0_0': "tiled_n8 | tiled nt2 | bf16",
        'n1_8-8_7x13x33_p8_8': "tiled_n8 | tiled_n8 | bf16",
        'n3_8-8_2x6x16_p0_0': "tiled_n8 | tiled_n8 | bf16",
        'n2_16-8_5x7x9_p0_0': "tiled_n8 | tiled nt1 | bf16",
    },
    ("N8_TILED", "f32"): {
        'n64_8-8_5x9x17_p0_0': "tiled_n8 | tiled_n8 | wgrad6 ci8 co8",
        'n64_16-8_5x9x17_p8_8': "tiled_n8 | tiled nt1 | wgrad6 co8",
        'n64_8-16_5x9x17_p0_8': "tiled nt1 | tiled_n8 | wgrad3",
        'n64_8-8_5x9x17_p8_8': "tiled_n8 | tiled_n8 | wgrad6 ci8 co8",
    },
    ("N8_TILED", "bf16"): {
        'n64_8-8_5x9x17_p0_0': "tiled_n8 | tiled_n8 | bf16",
        'n64_16-8_5x9x17_p8_8': "tiled_n8 | tiled nt1 | bf16",
        'n64_8-16_5x9x17_p0_8': "tiled nt1 | tiled_n8 | bf16",
        'n64_8-8_5x9x17_p8_8': "tiled_n8 | tiled_n8 | bf16",
    },
    ("STRIDED", "f32"): {
        'n1_8-16_16x18x20_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | wgrad3",
        'n1_16-32_9x11x13_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | wgrad6",
        'n2_32-64_10x12x9_p8_16': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | wgrad6",
        'n1_64-128_6x7x5_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | wgrad6",
        'n1_8-16_40x48x40_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split0 | wgrad3",
        'n3_24-40_5x6x33_p0_8': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | wgrad3",
        'n1_16-8_7x9x37_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | wgrad6 co8",
        'n1_8-16_2x3x1_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | wgrad3",
    },
    ("STRIDED", "bf16"): {
        'n1_8-16_16x18x20_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | bf16",
        'n1_16-32_9x11x13_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | bf16",
        'n2_32-64_10x12x9_p8_16': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | bf16",
        'n1_64-128_6x7x5_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | bf16",
        'n1_8-16_40x48x40_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split0 | bf16",
        'n3_24-40_5x6x33_p0_8': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | bf16",
        'n1_16-8_7x9x37_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | bf16",
        'n1_8-16_2x3x1_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | bf16",
    },
    ("STRIDED_WIDE", "f32"): {
        'n4_32-16_21x25x19_p0_0': "direct nt1 mode0 split1 | direct nt2 mode1 split0 | wgrad6",
        'n4_64-16_21x25x19_p0_8': "direct nt1 mode0 split1 | direct nt4 mode1 split0 | wgrad6",
        'n2_8-16_41x41x41_p0_0': "direct nt1 mode0 split0 | direct nt1 mode1 split0 | wgrad3",
        'n1_8-32_81x81x81_p0_0': "direct nt2 mode0 split0 | direct nt1 mode1 split0 | wgrad3",
        'n1_8-64_81x81x81_p0_0': "direct nt4 mode0 split0 | direct nt1 mode1 split0 | wgrad3",
    },
    ("STRIDED_WIDE", "bf16"): {
        'n4_32-16_21x25x19_p0_0': "direct nt1 mode0 split1 | direct nt2 mode1 split0 | bf16",
        'n4_64-16_21x25x19_p0_8': "direct nt1 mode0 split1 | direct nt4 mode1 split0 | bf16",
        'n2_8-16_41x41x41_p0_0': "direct nt1 mode0 split0 | direct nt1 mode1 split0 | bf16",
        'n1_8-32_81x81x81_p0_0': "direct nt2 mode0 split0 | direct nt1 mode1 split0 | bf16",
        'n1_8-64_81x81x81_p0_0': "direct nt4 mode0 split0 | direct nt1 mode1 split0 | bf16",
    },
    ("STRIDE3", "f32"): {
        'n1_16-32_10x11x13_p0_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | generic lds",
        'n2_8-16_7x8x19_p8_0': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | generic lds",
    },
    ("BF16_WGRAD_QUADS", "bf16"): {
        'n2_16-12_5x13x37_p0_0': "tiled nt1 | generic gather tl16 vec1 | wgrad4",
        'n2_16-20_5x9x17_p8_0': "tiled nt2 | generic gather tl16 vec1 | wgrad4",
        'n2_32-12_7x13x33_p0_0': "tiled nt1 | generic gather tl16 vec1 | wgrad4",
        'n2_16-16_5x13x37_p0_4': "tiled nt1 | generic gather tl16 vec1 | wgrad4",
        'n2_8-12_5x13x37_p0_0': "tiled nt1 | generic gather tl8 vec1 | wgrad3",
        'n2_24-20_5x9x17_p0_0': "tiled nt2 | generic gather tl16 vec1 | wgrad3",
    },
    ("MARCH_BF16", "bf16"): {
        'n48_16-16_41x5x9_p0_0': "march bias | march | bf16",
        'n48_16-16_41x9x17_p0_0': "march bias | march | bf16",
        'n48_32-16_41x5x9_p8_8': "march bias | march | bf16",
        'n48_16-48_41x5x9_p0_0': "tiled nt1 | march | bf16",
    },
    ("WGRAD_NOBIAS", "f32"): {
        'n2_8-12_5x13x37_p0_0': "direct nt1 mode0 split1 | generic gather tl8 vec1 | wgrad3",
        'n2_16-12_5x13x37_p0_0': "direct nt1 mode0 split1 | generic gather tl16 vec1 | wgrad6",
        'n1_8-8_7x13x33_p8_8': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 ci8 co8",
        'n1_32-8_11x19x37_p0_0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 co8",
        'n24_8-128_23x9x33_p8_0': "tiled nt2 | tiled_n8 | wgrad3",
    },
    ("WGRAD_NOBIAS", "bf16"): {
        'n2_8-12_5x13x37_p0_0': "tiled nt1 | generic gather tl8 vec1 | wgrad3",
        'n2_16-12_5x13x37_p0_0': "tiled nt1 | generic gather tl16 vec1 | wgrad4",
        'n1_8-8_7x13x33_p8_8': "tiled_n8 | tiled_n8 | bf16",
        'n1_32-8_11x19x37_p0_0': "tiled_n8 | tiled nt2 | bf16",
        'n24_8-128_23x9x33_p8_0': "tiled nt2 | tiled_n8 | bf16t",
    },
    ("MARCH_BF16_NOBIAS", "bf16"): {
        'n48_8-16_41x5x9_p0_0': "march | march | bf16",
    },
    ("STATS_ORACLE", "f32"): {
        'n2_16-16_5x9x17_b1': "tiled nt1 stats",
        'n2_8-32_5x9x17_b0': "tiled nt2 stats",
        'n48_16-16_41x5x9_b1': "tiled nt1 stats",
        'n48_8-16_41x5x9_b0': "tiled nt1 stats",
    },
    ("STATS_ORACLE", "bf16"): {
        'n2_16-16_5x9x17_b1': "tiled nt1 stats",
        'n2_8-32_5x9x17_b0': "tiled nt2 stats",
        'n48_16-16_41x5x9_b1': "march stats bias",
        'n48_8-16_41x5x9_b0': "march stats",
    },
    ("FIRST", "f32"): {
        'n2_1-8_9x13x37_b1_p0': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n1_1-16_8x16x32_b0_p0': "generic cin1 co16 | generic gather tl2 vec1 | cin1",
        'n1_1-8_4x8x32_b0_p8': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n3_1-16_5x7x19_b1_p0': "generic cin1 co16 | generic gather tl2 vec1 | cin1",
        'n1_1-8_1x1x1_b1_p0': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n1_1-8_17x9x70_b1_p8': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n2_1-16_6x20x33_b1_p16': "generic cin1 co16 | generic gather tl2 vec1 | cin1",
        'n1_1-8_12x24x64_b0_p0': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
    },
    ("FIRST", "bf16"): {
        'n2_1-8_9x13x37_b1_p0': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n1_1-16_8x16x32_b0_p0': "generic cin1 co16 | generic gather tl2 vec1 | cin1",
        'n1_1-8_4x8x32_b0_p8': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n3_1-16_5x7x19_b1_p0': "generic cin1 co16 | generic gather tl2 vec1 | cin1",
        'n1_1-8_1x1x1_b1_p0': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n1_1-8_17x9x70_b1_p8': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n2_1-16_6x20x33_b1_p16': "generic cin1 co16 | generic gather tl2 vec1 | cin1",
        'n1_1-8_12x24x64_b0_p0': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
    },
    ("ONE_OUT", "f32"): {
        'n2_8-1_k3x1x1_s111_9x13x37': "generic taps tl2 nt3 cv4 | generic taps tl8 nt3 cv1 | generic co1 ci8",
        'n1_1-1_k1x3x1_s111_4x8x32': "generic c1taps nt3 | generic c1taps nt3 | generic c1taps nt3",
        'n1_1-1_k1x1x3_s111_5x7x19': "generic taps tl2 nt3 cv1 | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n2_4-1_k1x6x1_s121_6x20x9': "generic taps tl2 nt6 cv4 | generic strided tl4 vec0 | generic co1 ci4",
        'n1_16-1_k1x1x3_s111_3x5x70': "generic taps tl2 nt3 cv4 | generic taps tl16 nt3 cv1 | generic co1 ci16",
        'n2_1-1_k3x3x3_s111_9x13x37': "generic c1c1 | generic c1c1 | generic c1c1",
        'n1_1-1_k3x3x3_s111_1x1x1': "generic c1c1 | generic c1c1 | generic c1c1",
        'n1_8-1_k6x1x1_s211_12x6x10': "generic taps tl2 nt6 cv4 | generic strided tl8 vec0 | generic co1 ci8",
    },
    ("OPS_CONV", "f32"): {
        'unet_1_8': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'unet_8_16': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad3",
        'unet_16_16': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'unet_16_32': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'unet_32_32': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'unet_32_64': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'unet_96_32': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'unet_48_16': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'unet_cls_16_2': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv1",
        'pw_32_2': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv1",
        'pw_64_8': "generic taps tl8 nt3 cv4 | pointwise co8 | pointwise co8 vx4 dv1",
        'pw_16_5': "generic taps tl8 nt3 cv4 | pointwise co8 | pointwise co8 vx4 dv0",
        'pw_128_64': "generic taps tl16 nt3 cv4 | generic taps tl16 nt3 cv4 | generic lds",
        'pw_8_3': "pointwise co4 | pointwise co4 | pointwise co4 vx4 dv0",
        'pw_4_1': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv0",
        'pw_64_4': "pointwise co4 | pointwise co4 | pointwise co4 vx4 dv1",
        'mfma_24_40': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad3",
        'mfma_64_128_ragged': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'ragged_3x3x3': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'tiny_1voxel': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad3",
        'sepx_k6s2p2': "generic taps tl8 nt6 cv1 | generic staps tl2 nt3 | generic quads nt8 civ1",
        'sepy_k6s2p2': "generic taps tl8 nt6 cv4 | generic staps tl8 nt3 | generic quads nt6 civ4",
        'sepz_k6s2p2': "generic taps tl16 nt6 cv4 | generic staps tl8 nt3 | generic quads nt6 civ4",
        'sepx_k3p0': "generic taps tl16 nt3 cv4 | generic taps tl16 nt3 cv4 | generic small",
        'sepz_k3p1': "generic taps tl8 nt3 cv4 | generic taps tl16 nt3 cv4 | generic quads nt4 civ4",
        'stride2_m3d': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | wgrad3",
        'stride2_odd': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | wgrad6",
        'dilated_s2': "generic gather tl4 vec0 | generic gather tl2 vec1 | generic lds",
        'dilated_p3': "generic gather tl4 vec1 | generic gather tl4 vec1 | generic lds",
        'reduce_k4s4': "generic gather tl2 vec0 | generic strided tl2 vec0 | generic lds",
        'vox_1_1': "generic c1c1 | generic c1c1 | generic c1c1",
        'c1_sepy': "generic c1taps nt3 | generic c1taps nt3 | generic c1taps nt3",
        'c1_sepz': "generic c1taps nt3 | generic c1taps nt3 | generic c1taps nt3",
        'c1_sepx_nobias': "generic c1taps nt3 | generic c1taps nt3 | generic c1taps nt3",
        'c1_sepz_k6_p2': "generic taps tl2 nt6 cv1 | generic taps tl2 nt8 cv1 | generic co1 ci1",
        'c1_sepz_k5_p2_dil2': "generic c1taps nt8 | generic c1taps nt8 | generic c1taps nt8",
        'c1_sepy_k2': "generic c1taps nt3 | generic c1taps nt3 | generic c1taps nt3",
        'c1_sepz_ragged': "generic taps tl2 nt3 cv1 | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'odd_channels': "generic gather tl8 vec0 | generic gather tl4 vec0 | generic lds",
        'wide_128': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
    },
    ("OPS_STATS", "f32"): {
        'n2_16-16_9x13x21_b1': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 | tiled nt1 stats",
        'n1_48-16_8x16x32_b1': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 | tiled nt1 stats",
        'n2_8-32_5x8x16_b0': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad3 | tiled nt2 stats",
        'n1_32-64_4x9x17_b1': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 | tiled nt2 stats",
        'n1_16-48_6x7x19_b1': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6 | tiled nt1 stats",
        'n64_16-16_9x13x21_b1': "tiled nt1 | tiled nt1 | wgrad6 | tiled nt1 stats",
        'n90_48-16_3x9x17_b0': "direct nt1 mode0 split0 | tiled nt1 | wgrad6 | tiled nt1 stats",
        'n88_16-48_5x7x19_b1': "tiled nt1 | direct nt1 mode0 split0 | wgrad6 | tiled nt1 stats",
    },
    ("OPS_STATS", "bf16"): {
        'n2_16-16_9x13x21_b1': "tiled nt1 | tiled nt1 | bf16 | tiled nt1 stats",
        'n1_48-16_8x16x32_b1': "tiled nt1 | tiled nt1 | bf16 | tiled nt1 stats",
        'n2_8-32_5x8x16_b0': "tiled nt2 | tiled_n8 | bf16 | tiled nt2 stats",
        'n1_32-64_4x9x17_b1': "tiled nt2 | tiled nt2 | bf16 | tiled nt2 stats",
        'n1_16-48_6x7x19_b1': "tiled nt1 | tiled nt1 | bf16 | tiled nt1 stats",
        'n64_16-16_9x13x21_b1': "tiled nt1 | tiled nt1 | bf16 | tiled nt1 stats",
        'n90_48-16_3x9x17_b0': "tiled nt1 | tiled nt1 | bf16 | tiled nt1 stats",
        'n88_16-48_5x7x19_b1': "tiled nt1 | tiled nt1 | bf16 | tiled nt1 stats",
    },
    ("CAT", "f32"): {
        'n2_16+32-16_24x40x70_p0_b1': "tiled nt1 | tiled nt1 stats | tiled nt1 | wgrad6",
        'n2_32+64-32_21x33x70_p8_b1': "tiled nt2 | tiled nt2 stats | tiled nt2 | wgrad6",
        'n8_32+64-32_45x17x37_p8_b1': "tiled nt2 | tiled nt2 stats | tiled nt2 | wgrad6",
        'n5_16+16-8_17x40x65_p0_b0': "tiled_n8 | tiled nt1 stats | tiled nt2 | wgrad6 co8",
        'n2_16+24-16_24x40x70_p0_b1': "tiled nt1 | tiled nt1 stats | tiled nt1 | none",
        'n1_8+16-16_24x40x70_p0_b1': "none | none | none | none",
        'n1_16+32-16_6x7x9_p0_b1': "none | none | none | wgrad6",
        'n5_16+16-16_17x40x65_p4_b1': "tiled nt1 | tiled nt1 stats | tiled nt2 | wgrad6",
    },
    ("CAT", "bf16"): {
        'n2_16+32-16_24x40x70_p0_b1': "tiled nt1 | tiled nt1 stats | tiled nt1 | bf16",
        'n2_32+64-32_21x33x70_p8_b1': "tiled nt2 | tiled nt2 stats | tiled nt2 | bf16",
        'n8_32+64-32_45x17x37_p8_b1': "tiled nt2 | tiled nt2 stats | tiled nt2 | bf16t",
        'n5_16+16-8_17x40x65_p0_b0': "tiled_n8 | tiled nt1 stats | tiled nt2 | bf16",
        'n2_16+24-16_24x40x70_p0_b1': "tiled nt1 | tiled nt1 stats | tiled nt1 | bf16",
        'n1_8+16-16_24x40x70_p0_b1': "none | none | none | none",
        'n1_16+32-16_6x7x9_p0_b1': "tiled nt1 | tiled nt1 stats | tiled nt1 | bf16",
        'n5_16+16-16_17x40x65_p4_b1': "none | none | tiled nt2 | none",
    },
    ("BF16_CONV", "bf16"): {
        'n2_8-16_12x20x18_k3_s1': "tiled nt1 | tiled_n8 | bf16",
        'n1_16-16_9x17x33_k3_s1': "tiled nt1 | tiled nt1 | bf16",
        'n1_48-16_8x16x16_k3_s1': "tiled nt1 | tiled nt1 | bf16",
        'n2_32-64_6x9x17_k3_s1': "tiled nt2 | tiled nt2 | bf16",
        'n1_96-32_5x8x16_k3_s1': "tiled nt2 | tiled nt2 | bf16",
        'n2_1-8_10x12x14_k3_s1': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n2_16-2_10x12x14_k1_s1': "pointwise co2 | pointwise co2 | pointwise co2 vx8 dv1",
        'n1_32-2_9x10x11_k1_s1': "pointwise co2 | pointwise co2 | pointwise co2 vx8 dv1",
        'n2_64-4_5x7x9_k1_s1': "pointwise co4 | pointwise co4 | pointwise co4 vx8 dv1",
        'n1_16-5_6x7x8_k1_s1': "generic taps tl8 nt3 cv4 | pointwise co8 | pointwise co8 vx4 dv0",
        'n1_24-3_6x7x8_k1_s1': "generic taps tl4 nt3 cv4 | generic gather tl16 vec0 | pointwise co4 vx4 dv0",
        'n1_8-16_11x12x13_k3_s2': "direct nt1 mode0 split1 | direct nt1 mode1 split1 | bf16",
        'n1_4-6_9x10x11_k(3, 1, 1)_s(2, 1, 1)': "generic taps tl8 nt3 cv4 | generic strided tl4 vec0 | generic small",
    },
    ("CAPI_STATS", "f32"): {
        'f32_tiled': "tiled nt2 stats",
        'f32_march': "march stats bias",
        'f32_cat_tiled': "tiled nt1 stats",
        'f32_cat_march': "march stats bias",
        'f32_cat_ld20': "tiled nt1 stats",
        'f32_cat_ld28': "tiled nt1 stats",
    },
    ("CAPI_STATS", "bf16"): {
        'bf16_tiled': "tiled nt2 stats",
        'bf16_march': "march stats bias",
        'bf16_cat_tiled': "tiled nt2 stats",
        'bf16_cat_march': "march stats bias",
    },
    ("WS_CONV", "f32"): {
        'conv_generic_odd_dilated': "generic gather tl8 vec0 | generic gather tl4 vec0 | generic lds",
        'conv_pointwise': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv1",
        'conv_small_f32': "direct nt1 mode0 split1 | direct nt1 mode0 split1 | wgrad6",
        'conv_narrow_f32': "direct nt1 mode0 split0 | direct nt1 mode0 split0 | wgrad6",
        'conv_tiled_f32': "tiled nt1 | tiled nt1 | wgrad6",
        'conv_march_f32': "march bias | march | wgrad6",
    },
    ("WS_CONV", "bf16"): {
        'conv_tiled_bf16': "tiled nt2 | tiled nt1 | bf16",
        'conv_n8_bf16': "tiled_n8 | tiled nt1 | bf16",
        'conv_march_bf16': "march bias | march | bf16",
        'conv_wgrad_bf16_march_d': "tiled nt2 | tiled nt2 | bf16t",
    },
    ("GENERIC_DENSE", "f32"): {
        'n1_1-1_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl2 nt3 cv1 | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n1_1-2_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic taps tl2 nt3 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-3_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl4 nt3 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-4_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl4 nt3 cv1 | generic taps tl2 nt3 cv4 | generic quads nt8 civ1",
        'n1_1-5_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic taps tl8 nt3 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-16_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl16 nt3 cv1 | generic taps tl2 nt3 cv4 | generic quads nt8 civ1",
        'n1_1-72_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl16 nt3 cv1 | generic taps tl2 nt3 cv4 | generic lds",
        'n1_2-1_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic gather tl2 vec0 | generic taps tl2 nt3 cv1 | generic small",
        'n1_2-3_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl4 vec0 | generic gather tl2 vec0 | generic small",
        'n1_2-5_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl8 vec0 | generic gather tl2 vec0 | generic small",
        'n1_2-16_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic gather tl16 vec0 | generic taps tl2 nt3 cv4 | generic small",
        'n1_3-1_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl2 vec0 | generic taps tl4 nt3 cv1 | generic small",
        'n1_3-2_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl2 vec0 | generic gather tl4 vec0 | generic small",
        'n1_3-4_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl4 vec0 | generic taps tl4 nt3 cv4 | generic small",
        'n1_4-1_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl2 nt3 cv4 | generic taps tl4 nt3 cv1 | generic co1 ci4",
        'n1_4-3_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl4 nt3 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-4_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl4 nt3 cv4 | generic taps tl4 nt3 cv4 | generic quads nt4 civ4",
        'n1_4-5_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic taps tl8 nt3 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-16_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl16 nt3 cv4 | generic taps tl4 nt3 cv4 | generic quads nt4 civ4",
        'n1_5-1_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic gather tl2 vec0 | generic taps tl8 nt3 cv1 | generic small",
        'n1_5-2_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl2 vec0 | generic gather tl8 vec0 | generic small",
        'n1_5-4_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic gather tl4 vec0 | generic taps tl8 nt3 cv4 | generic small",
        'n1_8-1_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic taps tl2 nt3 cv4 | generic taps tl8 nt3 cv1 | generic co1 ci8",
        'n1_16-1_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl2 nt3 cv4 | generic taps tl16 nt3 cv1 | generic co1 ci16",
        'n1_16-2_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic taps tl2 nt3 cv4 | generic gather tl16 vec0 | generic small",
        'n1_16-4_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl4 nt3 cv4 | generic taps tl16 nt3 cv4 | generic quads nt4 civ4",
        'n1_1-1_5x7x8_k211_s111_p100_d111_b1_i0_o0': "generic c1taps nt3 | generic c1taps nt3 | generic c1taps nt3",
        'n1_1-1_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic taps tl2 nt3 cv1 | generic strided tl2 vec0 | generic co1 ci1",
        'n1_1-4_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic taps tl4 nt3 cv1 | generic staps tl2 nt3 | generic quads nt8 civ1",
        'n1_3-1_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic gather tl2 vec0 | generic strided tl4 vec0 | generic small",
        'n1_3-4_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic gather tl4 vec0 | generic staps tl4 nt3 | generic small",
        'n1_5-1_5x7x9_k211_s211_p000_d111_b0_i0_o0': "generic gather tl2 vec0 | generic strided tl8 vec0 | generic small",
        'n1_5-4_5x7x9_k211_s211_p000_d111_b0_i0_o0': "generic gather tl4 vec0 | generic staps tl8 nt3 | generic small",
        'n1_16-1_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic taps tl2 nt3 cv4 | generic strided tl16 vec0 | generic co1 ci16",
        'n1_16-4_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic taps tl4 nt3 cv4 | generic staps tl16 nt3 | generic quads nt4 civ4",
        'n1_1-1_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl2 nt6 cv1 | generic taps tl2 nt8 cv1 | generic co1 ci1",
        'n1_1-3_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-4_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv1 | generic taps tl2 nt4 cv4 | generic quads nt8 civ1",
        'n1_1-5_5x7x9_k411_s111_p200_d111_b0_i0_o0': "generic taps tl8 nt6 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-16_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl16 nt6 cv1 | generic taps tl2 nt4 cv4 | generic quads nt8 civ1",
        'n1_3-1_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic gather tl2 vec0 | generic taps tl4 nt8 cv1 | generic small",
        'n1_3-4_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic gather tl4 vec0 | generic taps tl4 nt4 cv4 | generic small",
        'n1_4-1_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl2 nt4 cv4 | generic taps tl4 nt8 cv1 | generic co1 ci4",
        'n1_4-3_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt4 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-5_5x7x9_k411_s111_p200_d111_b0_i0_o0': "generic taps tl8 nt4 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-16_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl16 nt4 cv4 | generic taps tl4 nt4 cv4 | generic quads nt4 civ4",
        'n1_5-1_5x7x9_k411_s111_p200_d111_b0_i0_o0': "generic gather tl2 vec0 | generic taps tl8 nt8 cv1 | generic small",
        'n1_5-4_5x7x9_k411_s111_p200_d111_b0_i0_o0': "generic gather tl4 vec0 | generic taps tl8 nt4 cv4 | generic small",
        'n1_16-1_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl2 nt4 cv4 | generic taps tl16 nt8 cv1 | generic co1 ci16",
        'n1_16-4_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt4 cv4 | generic taps tl16 nt4 cv4 | generic quads nt4 civ4",
        'n1_1-1_5x7x8_k411_s111_p200_d111_b1_i0_o0': "generic c1taps nt8 | generic c1taps nt8 | generic c1taps nt8",
        'n1_1-4_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv1 | generic taps tl2 nt6 cv4 | generic quads nt8 civ1",
        'n1_3-4_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic gather tl4 vec0 | generic taps tl4 nt6 cv4 | generic small",
        'n1_4-1_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl2 nt6 cv4 | generic taps tl4 nt8 cv1 | generic co1 ci4",
        'n1_4-3_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-4_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv4 | generic taps tl4 nt6 cv4 | generic quads nt6 civ4",
        'n1_4-5_5x7x9_k511_s111_p200_d111_b0_i0_o0': "generic taps tl8 nt6 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-16_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl16 nt6 cv4 | generic taps tl4 nt6 cv4 | generic quads nt6 civ4",
        'n1_5-4_5x7x9_k511_s111_p200_d111_b0_i0_o0': "generic gather tl4 vec0 | generic taps tl8 nt6 cv4 | generic small",
        'n1_16-4_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv4 | generic taps tl16 nt6 cv4 | generic quads nt6 civ4",
        'n1_1-1_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl2 nt8 cv1 | generic taps tl2 nt8 cv1 | generic co1 ci1",
        'n1_1-3_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl4 nt8 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-4_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl4 nt8 cv1 | generic taps tl2 nt8 cv4 | generic quads nt8 civ1",
        'n1_1-5_5x7x9_k222_s111_p000_d111_b0_i0_o0': "generic taps tl8 nt8 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-16_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl16 nt8 cv1 | generic taps tl2 nt8 cv4 | generic quads nt8 civ1",
        'n1_3-4_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic gather tl4 vec0 | generic taps tl4 nt8 cv4 | generic small",
        'n1_4-1_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl2 nt8 cv4 | generic taps tl4 nt8 cv1 | generic co1 ci4",
        'n1_4-3_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl4 nt8 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-4_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl4 nt8 cv4 | generic taps tl4 nt8 cv4 | generic quads nt8 civ4",
        'n1_4-5_5x7x9_k222_s111_p000_d111_b0_i0_o0': "generic taps tl8 nt8 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-16_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl16 nt8 cv4 | generic taps tl4 nt8 cv4 | generic quads nt8 civ4",
        'n1_5-4_5x7x9_k222_s111_p000_d111_b0_i0_o0': "generic gather tl4 vec0 | generic taps tl8 nt8 cv4 | generic small",
        'n1_16-4_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl4 nt8 cv4 | generic taps tl16 nt8 cv4 | generic quads nt8 civ4",
        'n1_1-4_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl4 vec0 | generic staps tl2 nt4 | generic lds",
        'n1_3-4_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl4 vec0 | generic staps tl4 nt4 | generic lds",
        'n1_4-1_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl2 vec1 | generic strided tl4 vec0 | generic lds",
        'n1_4-3_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl4 vec1 | generic strided tl4 vec0 | generic lds",
        'n1_4-5_5x7x9_k331_s221_p110_d111_b0_i0_o0': "generic gather tl8 vec1 | generic strided tl4 vec0 | generic lds",
        'n1_4-16_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl16 vec1 | generic staps tl4 nt4 | generic lds",
        'n1_5-4_5x7x9_k331_s221_p110_d111_b0_i0_o0': "generic gather tl4 vec0 | generic staps tl8 nt4 | generic lds",
        'n1_16-4_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl4 vec1 | generic staps tl16 nt4 | generic lds",
        'n1_1-4_5x7x9_k444_s222_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic staps tl2 nt8 | generic lds",
        'n1_3-4_5x7x9_k444_s222_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic staps tl4 nt8 | generic lds",
        'n1_5-4_5x7x9_k444_s222_p111_d111_b0_i0_o0': "generic gather tl4 vec0 | generic staps tl8 nt8 | generic lds",
        'n1_16-4_5x7x9_k444_s222_p111_d111_b1_i0_o0': "generic gather tl4 vec1 | generic staps tl16 nt8 | generic lds",
        'n1_1-1_5x7x9_k333_s111_p111_d111_b1_i0_o0': "generic c1c1 | generic c1c1 | generic c1c1",
        'n1_1-4_5x7x9_k333_s111_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic gather tl2 vec1 | cin1",
        'n1_1-8_5x7x9_k333_s111_p111_d111_b0_i0_o0': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n1_1-16_5x7x9_k333_s111_p111_d111_b1_i0_o0': "generic cin1 co16 | generic gather tl2 vec1 | cin1",
        'n1_3-4_5x7x9_k333_s111_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic gather tl4 vec1 | generic lds",
        'n1_5-4_5x7x9_k333_s111_p111_d111_b0_i0_o0': "generic gather tl4 vec0 | generic gather tl8 vec1 | generic lds",
        'n1_16-4_5x7x9_k333_s111_p111_d111_b1_i0_o0': "generic gather tl4 vec1 | generic gather tl16 vec1 | wgrad6",
        'n1_1-4_5x7x9_k333_s211_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic strided tl2 vec1 | generic lds",
        'n1_3-4_5x7x9_k333_s211_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic strided tl4 vec1 | generic lds",
        'n1_5-4_5x7x9_k333_s211_p111_d111_b0_i0_o0': "generic gather tl4 vec0 | generic strided tl8 vec1 | generic lds",
        'n1_16-4_5x7x9_k333_s211_p111_d111_b1_i0_o0': "generic gather tl4 vec1 | generic strided tl16 vec1 | generic lds",
        'n1_4-1_5x7x9_k111_s111_p000_d111_b1_i0_o0': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv0",
        'n1_4-2_5x7x9_k111_s111_p000_d111_b0_i0_o0': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv1",
        'n1_4-3_5x7x9_k111_s111_p000_d111_b1_i0_o0': "pointwise co4 | pointwise co4 | pointwise co4 vx4 dv0",
        'n1_4-4_5x7x9_k111_s111_p000_d111_b1_i0_o0': "pointwise co4 | pointwise co4 | pointwise co4 vx4 dv1",
        'n1_4-5_5x7x9_k111_s111_p000_d111_b0_i0_o0': "generic taps tl8 nt3 cv4 | pointwise co8 | pointwise co8 vx4 dv0",
        'n1_4-8_5x7x9_k111_s111_p000_d111_b0_i0_o0': "generic taps tl8 nt3 cv4 | pointwise co8 | pointwise co8 vx4 dv1",
        'n1_8-1_5x7x9_k111_s111_p000_d111_b0_i0_o0': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv0",
        'n1_8-2_5x7x9_k111_s111_p000_d111_b1_i0_o0': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv1",
        'n1_8-3_5x7x9_k111_s111_p000_d111_b1_i0_o0': "pointwise co4 | pointwise co4 | pointwise co4 vx4 dv0",
        'n1_8-4_5x7x9_k111_s111_p000_d111_b0_i0_o0': "pointwise co4 | pointwise co4 | pointwise co4 vx4 dv1",
        'n1_8-8_1x7x9_k131_s111_p010_d111_b1_i0_o0': "generic taps tl8 nt3 cv4 | generic taps tl8 nt3 cv4 | generic quads nt4 civ4",
        'n2_16-8_3x5x70_k116_s112_p002_d111_b1_i0_o0': "generic taps tl8 nt6 cv4 | generic staps tl16 nt3 | generic quads nt6 civ4",
        'n1_1-1_5x1x9_k333_s111_p111_d111_b1_i0_o0': "generic c1c1 | generic c1c1 | generic c1c1",
        'n3_4-4_5x7x1_k222_s111_p111_d111_b0_i0_o0': "generic taps tl4 nt8 cv4 | generic taps tl4 nt8 cv4 | generic quads nt8 civ4",
        'n1_8-16_9x1x33_k611_s211_p200_d111_b1_i0_o0': "generic taps tl16 nt6 cv4 | generic staps tl8 nt3 | generic quads nt6 civ4",
    },
    ("GENERIC_DENSE", "bf16"): {
        'n1_1-1_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl2 nt3 cv1 | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n1_1-2_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic taps tl2 nt3 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-3_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl4 nt3 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-4_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl4 nt3 cv1 | generic taps tl2 nt3 cv4 | generic quads nt8 civ1",
        'n1_1-5_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic taps tl8 nt3 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-16_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl16 nt3 cv1 | generic taps tl2 nt3 cv4 | generic quads nt8 civ1",
        'n1_1-72_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl16 nt3 cv1 | generic taps tl2 nt3 cv4 | generic lds",
        'n1_2-1_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic gather tl2 vec0 | generic taps tl2 nt3 cv1 | generic small",
        'n1_2-3_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl4 vec0 | generic gather tl2 vec0 | generic small",
        'n1_2-5_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl8 vec0 | generic gather tl2 vec0 | generic small",
        'n1_2-16_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic gather tl16 vec0 | generic taps tl2 nt3 cv4 | generic small",
        'n1_3-1_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl2 vec0 | generic taps tl4 nt3 cv1 | generic small",
        'n1_3-2_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl2 vec0 | generic gather tl4 vec0 | generic small",
        'n1_3-4_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl4 vec0 | generic taps tl4 nt3 cv4 | generic small",
        'n1_4-1_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl2 nt3 cv4 | generic taps tl4 nt3 cv1 | generic co1 ci4",
        'n1_4-3_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl4 nt3 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-4_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl4 nt3 cv4 | generic taps tl4 nt3 cv4 | generic quads nt4 civ4",
        'n1_4-5_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic taps tl8 nt3 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-16_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl16 nt3 cv4 | generic taps tl4 nt3 cv4 | generic quads nt4 civ4",
        'n1_5-1_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic gather tl2 vec0 | generic taps tl8 nt3 cv1 | generic small",
        'n1_5-2_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic gather tl2 vec0 | generic gather tl8 vec0 | generic small",
        'n1_5-4_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic gather tl4 vec0 | generic taps tl8 nt3 cv4 | generic small",
        'n1_8-1_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic taps tl2 nt3 cv4 | generic taps tl8 nt3 cv1 | generic co1 ci8",
        'n1_16-1_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl2 nt3 cv4 | generic taps tl16 nt3 cv1 | generic co1 ci16",
        'n1_16-2_5x7x9_k211_s111_p100_d111_b0_i0_o0': "generic taps tl2 nt3 cv4 | generic gather tl16 vec0 | generic small",
        'n1_16-4_5x7x9_k211_s111_p100_d111_b1_i0_o0': "generic taps tl4 nt3 cv4 | generic taps tl16 nt3 cv4 | generic quads nt4 civ4",
        'n1_1-1_5x7x8_k211_s111_p100_d111_b1_i0_o0': "generic taps tl2 nt3 cv1 | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n1_1-1_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic taps tl2 nt3 cv1 | generic strided tl2 vec0 | generic co1 ci1",
        'n1_1-4_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic taps tl4 nt3 cv1 | generic staps tl2 nt3 | generic quads nt8 civ1",
        'n1_3-1_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic gather tl2 vec0 | generic strided tl4 vec0 | generic small",
        'n1_3-4_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic gather tl4 vec0 | generic staps tl4 nt3 | generic small",
        'n1_5-1_5x7x9_k211_s211_p000_d111_b0_i0_o0': "generic gather tl2 vec0 | generic strided tl8 vec0 | generic small",
        'n1_5-4_5x7x9_k211_s211_p000_d111_b0_i0_o0': "generic gather tl4 vec0 | generic staps tl8 nt3 | generic small",
        'n1_16-1_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic taps tl2 nt3 cv4 | generic strided tl16 vec0 | generic co1 ci16",
        'n1_16-4_5x7x9_k211_s211_p000_d111_b1_i0_o0': "generic taps tl4 nt3 cv4 | generic staps tl16 nt3 | generic quads nt4 civ4",
        'n1_1-1_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl2 nt6 cv1 | generic taps tl2 nt8 cv1 | generic co1 ci1",
        'n1_1-3_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-4_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv1 | generic taps tl2 nt4 cv4 | generic quads nt8 civ1",
        'n1_1-5_5x7x9_k411_s111_p200_d111_b0_i0_o0': "generic taps tl8 nt6 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-16_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl16 nt6 cv1 | generic taps tl2 nt4 cv4 | generic quads nt8 civ1",
        'n1_3-1_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic gather tl2 vec0 | generic taps tl4 nt8 cv1 | generic small",
        'n1_3-4_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic gather tl4 vec0 | generic taps tl4 nt4 cv4 | generic small",
        'n1_4-1_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl2 nt4 cv4 | generic taps tl4 nt8 cv1 | generic co1 ci4",
        'n1_4-3_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt4 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-5_5x7x9_k411_s111_p200_d111_b0_i0_o0': "generic taps tl8 nt4 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-16_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl16 nt4 cv4 | generic taps tl4 nt4 cv4 | generic quads nt4 civ4",
        'n1_5-1_5x7x9_k411_s111_p200_d111_b0_i0_o0': "generic gather tl2 vec0 | generic taps tl8 nt8 cv1 | generic small",
        'n1_5-4_5x7x9_k411_s111_p200_d111_b0_i0_o0': "generic gather tl4 vec0 | generic taps tl8 nt4 cv4 | generic small",
        'n1_16-1_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl2 nt4 cv4 | generic taps tl16 nt8 cv1 | generic co1 ci16",
        'n1_16-4_5x7x9_k411_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt4 cv4 | generic taps tl16 nt4 cv4 | generic quads nt4 civ4",
        'n1_1-1_5x7x8_k411_s111_p200_d111_b1_i0_o0': "generic taps tl2 nt6 cv1 | generic taps tl2 nt8 cv1 | generic co1 ci1",
        'n1_1-4_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv1 | generic taps tl2 nt6 cv4 | generic quads nt8 civ1",
        'n1_3-4_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic gather tl4 vec0 | generic taps tl4 nt6 cv4 | generic small",
        'n1_4-1_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl2 nt6 cv4 | generic taps tl4 nt8 cv1 | generic co1 ci4",
        'n1_4-3_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-4_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv4 | generic taps tl4 nt6 cv4 | generic quads nt6 civ4",
        'n1_4-5_5x7x9_k511_s111_p200_d111_b0_i0_o0': "generic taps tl8 nt6 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-16_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl16 nt6 cv4 | generic taps tl4 nt6 cv4 | generic quads nt6 civ4",
        'n1_5-4_5x7x9_k511_s111_p200_d111_b0_i0_o0': "generic gather tl4 vec0 | generic taps tl8 nt6 cv4 | generic small",
        'n1_16-4_5x7x9_k511_s111_p200_d111_b1_i0_o0': "generic taps tl4 nt6 cv4 | generic taps tl16 nt6 cv4 | generic quads nt6 civ4",
        'n1_1-1_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl2 nt8 cv1 | generic taps tl2 nt8 cv1 | generic co1 ci1",
        'n1_1-3_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl4 nt8 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-4_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl4 nt8 cv1 | generic taps tl2 nt8 cv4 | generic quads nt8 civ1",
        'n1_1-5_5x7x9_k222_s111_p000_d111_b0_i0_o0': "generic taps tl8 nt8 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-16_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl16 nt8 cv1 | generic taps tl2 nt8 cv4 | generic quads nt8 civ1",
        'n1_3-4_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic gather tl4 vec0 | generic taps tl4 nt8 cv4 | generic small",
        'n1_4-1_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl2 nt8 cv4 | generic taps tl4 nt8 cv1 | generic co1 ci4",
        'n1_4-3_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl4 nt8 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-4_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl4 nt8 cv4 | generic taps tl4 nt8 cv4 | generic quads nt8 civ4",
        'n1_4-5_5x7x9_k222_s111_p000_d111_b0_i0_o0': "generic taps tl8 nt8 cv4 | generic gather tl4 vec0 | generic small",
        'n1_4-16_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl16 nt8 cv4 | generic taps tl4 nt8 cv4 | generic quads nt8 civ4",
        'n1_5-4_5x7x9_k222_s111_p000_d111_b0_i0_o0': "generic gather tl4 vec0 | generic taps tl8 nt8 cv4 | generic small",
        'n1_16-4_5x7x9_k222_s111_p000_d111_b1_i0_o0': "generic taps tl4 nt8 cv4 | generic taps tl16 nt8 cv4 | generic quads nt8 civ4",
        'n1_1-4_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl4 vec0 | generic staps tl2 nt4 | generic lds",
        'n1_3-4_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl4 vec0 | generic staps tl4 nt4 | generic lds",
        'n1_4-1_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl2 vec1 | generic strided tl4 vec0 | generic lds",
        'n1_4-3_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl4 vec1 | generic strided tl4 vec0 | generic lds",
        'n1_4-5_5x7x9_k331_s221_p110_d111_b0_i0_o0': "generic gather tl8 vec1 | generic strided tl4 vec0 | generic lds",
        'n1_4-16_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl16 vec1 | generic staps tl4 nt4 | generic lds",
        'n1_5-4_5x7x9_k331_s221_p110_d111_b0_i0_o0': "generic gather tl4 vec0 | generic staps tl8 nt4 | generic lds",
        'n1_16-4_5x7x9_k331_s221_p110_d111_b1_i0_o0': "generic gather tl4 vec1 | generic staps tl16 nt4 | generic lds",
        'n1_1-4_5x7x9_k444_s222_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic staps tl2 nt8 | generic lds",
        'n1_3-4_5x7x9_k444_s222_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic staps tl4 nt8 | generic lds",
        'n1_5-4_5x7x9_k444_s222_p111_d111_b0_i0_o0': "generic gather tl4 vec0 | generic staps tl8 nt8 | generic lds",
        'n1_16-4_5x7x9_k444_s222_p111_d111_b1_i0_o0': "generic gather tl4 vec1 | generic staps tl16 nt8 | generic lds",
        'n1_1-1_5x7x9_k333_s111_p111_d111_b1_i0_o0': "generic c1c1 | generic c1c1 | generic c1c1",
        'n1_1-4_5x7x9_k333_s111_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic gather tl2 vec1 | cin1",
        'n1_1-8_5x7x9_k333_s111_p111_d111_b0_i0_o0': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n1_1-16_5x7x9_k333_s111_p111_d111_b1_i0_o0': "generic cin1 co16 | generic gather tl2 vec1 | cin1",
        'n1_3-4_5x7x9_k333_s111_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic gather tl4 vec1 | generic lds",
        'n1_5-4_5x7x9_k333_s111_p111_d111_b0_i0_o0': "generic gather tl4 vec0 | generic gather tl8 vec1 | generic lds",
        'n1_16-4_5x7x9_k333_s111_p111_d111_b1_i0_o0': "generic gather tl4 vec1 | generic gather tl16 vec1 | wgrad4",
        'n1_1-4_5x7x9_k333_s211_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic strided tl2 vec1 | generic lds",
        'n1_3-4_5x7x9_k333_s211_p111_d111_b1_i0_o0': "generic gather tl4 vec0 | generic strided tl4 vec1 | generic lds",
        'n1_5-4_5x7x9_k333_s211_p111_d111_b0_i0_o0': "generic gather tl4 vec0 | generic strided tl8 vec1 | generic lds",
        'n1_16-4_5x7x9_k333_s211_p111_d111_b1_i0_o0': "generic gather tl4 vec1 | generic strided tl16 vec1 | generic lds",
        'n1_4-1_5x7x9_k111_s111_p000_d111_b1_i0_o0': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv0",
        'n1_4-2_5x7x9_k111_s111_p000_d111_b0_i0_o0': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv1",
        'n1_4-3_5x7x9_k111_s111_p000_d111_b1_i0_o0': "pointwise co4 | pointwise co4 | pointwise co4 vx4 dv0",
        'n1_4-4_5x7x9_k111_s111_p000_d111_b1_i0_o0': "pointwise co4 | pointwise co4 | pointwise co4 vx4 dv1",
        'n1_4-5_5x7x9_k111_s111_p000_d111_b0_i0_o0': "generic taps tl8 nt3 cv4 | pointwise co8 | pointwise co8 vx4 dv0",
        'n1_4-8_5x7x9_k111_s111_p000_d111_b0_i0_o0': "generic taps tl8 nt3 cv4 | pointwise co8 | pointwise co8 vx4 dv1",
        'n1_8-1_5x7x9_k111_s111_p000_d111_b0_i0_o0': "pointwise co2 | pointwise co2 | pointwise co2 vx8 dv0",
        'n1_8-2_5x7x9_k111_s111_p000_d111_b1_i0_o0': "pointwise co2 | pointwise co2 | pointwise co2 vx8 dv1",
        'n1_8-3_5x7x9_k111_s111_p000_d111_b1_i0_o0': "pointwise co4 | pointwise co4 | pointwise co4 vx8 dv0",
        'n1_8-4_5x7x9_k111_s111_p000_d111_b0_i0_o0': "pointwise co4 | pointwise co4 | pointwise co4 vx8 dv1",
        'n1_8-8_1x7x9_k131_s111_p010_d111_b1_i0_o0': "generic taps tl8 nt3 cv4 | generic taps tl8 nt3 cv4 | generic quads nt4 civ4",
        'n2_16-8_3x5x70_k116_s112_p002_d111_b1_i0_o0': "generic taps tl8 nt6 cv4 | generic staps tl16 nt3 | generic quads nt6 civ4",
        'n1_1-1_5x1x9_k333_s111_p111_d111_b1_i0_o0': "generic c1c1 | generic c1c1 | generic c1c1",
        'n3_4-4_5x7x1_k222_s111_p111_d111_b0_i0_o0': "generic taps tl4 nt8 cv4 | generic taps tl4 nt8 cv4 | generic quads nt8 civ4",
        'n1_8-16_9x1x33_k611_s211_p200_d111_b1_i0_o0': "generic taps tl16 nt6 cv4 | generic staps tl8 nt3 | generic quads nt6 civ4",
    },
    ("GENERIC_PITCHED", "f32"): {
        'n1_1-1_5x7x9_k211_s111_p100_d111_b1_i4_o4': "generic taps tl2 nt3 cv1 | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n1_1-2_5x7x9_k211_s111_p100_d111_b0_i4_o4': "generic taps tl2 nt3 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-4_5x7x9_k211_s111_p100_d111_b1_i4_o4': "generic taps tl4 nt3 cv1 | generic taps tl2 nt3 cv4 | generic quads nt8 civ1",
        'n1_1-72_5x7x9_k211_s111_p100_d111_b1_i4_o4': "generic taps tl16 nt3 cv1 | generic taps tl2 nt3 cv4 | generic lds",
        'n1_2-1_5x7x9_k211_s111_p100_d111_b0_i4_o4': "generic gather tl2 vec0 | generic taps tl2 nt3 cv1 | generic small",
        'n1_1-1_5x7x9_k211_s211_p000_d111_b1_i4_o4': "generic taps tl2 nt3 cv1 | generic strided tl2 vec0 | generic co1 ci1",
        'n1_1-4_5x7x9_k211_s211_p000_d111_b1_i4_o4': "generic taps tl4 nt3 cv1 | generic staps tl2 nt3 | generic quads nt8 civ1",
        'n1_1-1_5x7x9_k333_s111_p111_d111_b1_i4_o4': "generic c1c1 | generic c1c1 | generic c1c1",
        'n1_1-8_5x7x9_k333_s111_p111_d111_b0_i4_o4': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n1_1-16_5x7x9_k333_s111_p111_d111_b1_i4_o4': "generic cin1 co16 | generic gather tl2 vec1 | cin1",
        'n1_4-1_5x7x9_k111_s111_p000_d111_b1_i4_o4': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv0",
        'n1_1-1_5x7x9_k211_s111_p100_d111_b1_i1_o1': "generic taps tl2 nt3 cv1 | generic taps tl2 nt3 cv1 | generic small",
        'n1_1-2_5x7x9_k211_s111_p100_d111_b0_i1_o1': "generic taps tl2 nt3 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-72_5x7x9_k211_s111_p100_d111_b1_i1_o1': "generic taps tl16 nt3 cv1 | generic gather tl2 vec0 | generic lds",
        'n1_2-1_5x7x9_k211_s111_p100_d111_b0_i1_o1': "generic gather tl2 vec0 | generic taps tl2 nt3 cv1 | generic small",
        'n1_1-1_5x7x9_k211_s211_p000_d111_b1_i1_o1': "generic taps tl2 nt3 cv1 | generic strided tl2 vec0 | generic small",
        'n1_1-1_5x7x9_k333_s111_p111_d111_b1_i1_o1': "generic c1c1 | generic c1c1 | generic c1c1",
        'n1_1-8_5x7x9_k333_s111_p111_d111_b0_i1_o1': "generic cin1 co8 | generic gather tl2 vec0 | generic lds",
        'n1_4-1_5x7x9_k111_s111_p000_d111_b1_i1_o1': "generic gather tl2 vec0 | pointwise co2 | generic small",
        'n1_1-16_5x7x9_k333_s111_p111_d111_b1_i1_o0': "generic cin1 co16 | generic gather tl2 vec1 | generic cin1 co16",
        'n1_8-8_5x7x70_k113_s111_p001_d111_b1_i4_o4': "generic taps tl8 nt3 cv4 | generic taps tl8 nt3 cv4 | generic quads nt4 civ4",
        'n2_1-8_1x9x13_k333_s111_p111_d111_b1_i0_o4': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n1_16-2_3x1x11_k111_s111_p000_d111_b1_i4_o0': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv1",
    },
    ("GENERIC_PITCHED", "bf16"): {
        'n1_1-1_5x7x9_k211_s111_p100_d111_b1_i4_o4': "generic taps tl2 nt3 cv1 | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n1_1-2_5x7x9_k211_s111_p100_d111_b0_i4_o4': "generic taps tl2 nt3 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-4_5x7x9_k211_s111_p100_d111_b1_i4_o4': "generic taps tl4 nt3 cv1 | generic taps tl2 nt3 cv4 | generic quads nt8 civ1",
        'n1_1-72_5x7x9_k211_s111_p100_d111_b1_i4_o4': "generic taps tl16 nt3 cv1 | generic taps tl2 nt3 cv4 | generic lds",
        'n1_2-1_5x7x9_k211_s111_p100_d111_b0_i4_o4': "generic gather tl2 vec0 | generic taps tl2 nt3 cv1 | generic small",
        'n1_1-1_5x7x9_k211_s211_p000_d111_b1_i4_o4': "generic taps tl2 nt3 cv1 | generic strided tl2 vec0 | generic co1 ci1",
        'n1_1-4_5x7x9_k211_s211_p000_d111_b1_i4_o4': "generic taps tl4 nt3 cv1 | generic staps tl2 nt3 | generic quads nt8 civ1",
        'n1_1-1_5x7x9_k333_s111_p111_d111_b1_i4_o4': "generic c1c1 | generic c1c1 | generic c1c1",
        'n1_1-8_5x7x9_k333_s111_p111_d111_b0_i4_o4': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n1_1-16_5x7x9_k333_s111_p111_d111_b1_i4_o4': "generic cin1 co16 | generic gather tl2 vec1 | generic cin1 co16",
        'n1_4-1_5x7x9_k111_s111_p000_d111_b1_i4_o4': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv0",
        'n1_1-1_5x7x9_k211_s111_p100_d111_b1_i1_o1': "generic taps tl2 nt3 cv1 | generic taps tl2 nt3 cv1 | generic small",
        'n1_1-2_5x7x9_k211_s111_p100_d111_b0_i1_o1': "generic taps tl2 nt3 cv1 | generic gather tl2 vec0 | generic small",
        'n1_1-72_5x7x9_k211_s111_p100_d111_b1_i1_o1': "generic taps tl16 nt3 cv1 | generic gather tl2 vec0 | generic lds",
        'n1_2-1_5x7x9_k211_s111_p100_d111_b0_i1_o1': "generic gather tl2 vec0 | generic taps tl2 nt3 cv1 | generic small",
        'n1_1-1_5x7x9_k211_s211_p000_d111_b1_i1_o1': "generic taps tl2 nt3 cv1 | generic strided tl2 vec0 | generic small",
        'n1_1-1_5x7x9_k333_s111_p111_d111_b1_i1_o1': "generic c1c1 | generic c1c1 | generic c1c1",
        'n1_1-8_5x7x9_k333_s111_p111_d111_b0_i1_o1': "generic cin1 co8 | generic gather tl2 vec0 | generic lds",
        'n1_4-1_5x7x9_k111_s111_p000_d111_b1_i1_o1': "generic gather tl2 vec0 | pointwise co2 | generic small",
        'n1_1-16_5x7x9_k333_s111_p111_d111_b1_i1_o0': "generic cin1 co16 | generic gather tl2 vec1 | generic cin1 co16",
        'n1_8-8_5x7x70_k113_s111_p001_d111_b1_i4_o4': "generic taps tl8 nt3 cv4 | generic taps tl8 nt3 cv4 | generic quads nt4 civ4",
        'n2_1-8_1x9x13_k333_s111_p111_d111_b1_i0_o4': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'n1_16-2_3x1x11_k111_s111_p000_d111_b1_i4_o0': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv1",
    },
    ("TRANSPOSE", "f32"): {
        'n1_1-1_2x3x17_k211_s111_p000_o000_b1': "generic taps tl2 nt3 cv1 bias | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n1_1-3_2x3x17_k211_s111_p000_o000_b1': "generic taps tl4 nt3 cv1 bias | generic gather tl2 vec0 | generic small",
        'n1_1-5_2x3x17_k211_s111_p000_o000_b1': "generic taps tl8 nt3 cv1 bias | generic gather tl2 vec0 | generic small",
        'n1_1-16_2x3x17_k211_s111_p000_o000_b1': "generic taps tl16 nt3 cv1 bias | generic taps tl2 nt3 cv4 | generic co1 ci16",
        'n1_2-1_2x3x17_k211_s111_p000_o000_b1': "generic gather tl2 vec0 bias | generic taps tl2 nt3 cv1 | generic small",
        'n1_2-3_2x3x17_k211_s111_p000_o000_b1': "generic gather tl4 vec0 bias | generic gather tl2 vec0 | generic small",
        'n1_2-5_2x3x17_k211_s111_p000_o000_b1': "generic gather tl8 vec0 bias | generic gather tl2 vec0 | generic small",
        'n1_2-16_2x3x17_k211_s111_p000_o000_b1': "generic gather tl16 vec0 bias | generic taps tl2 nt3 cv4 | generic small",
        'n1_4-1_2x3x17_k211_s111_p000_o000_b1': "generic taps tl2 nt3 cv4 bias | generic taps tl4 nt3 cv1 | generic quads nt8 civ1",
        'n1_4-3_2x3x17_k211_s111_p000_o000_b1': "generic taps tl4 nt3 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-5_2x3x17_k211_s111_p000_o000_b1': "generic taps tl8 nt3 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-16_2x3x17_k211_s111_p000_o000_b1': "generic taps tl16 nt3 cv4 bias | generic taps tl4 nt3 cv4 | generic quads nt4 civ4",
        'n2_1-1_3x5x7_k211_s211_p000_o100_b1': "generic strided tl2 vec0 bias | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n2_1-3_3x5x7_k211_s211_p000_o100_b1': "generic strided tl4 vec0 bias | generic gather tl2 vec0 | generic small",
        'n2_1-5_3x5x7_k211_s211_p000_o100_b1': "generic strided tl8 vec0 bias | generic gather tl2 vec0 | generic small",
        'n2_1-16_3x5x7_k211_s211_p000_o100_b1': "generic strided tl16 vec0 bias | generic taps tl2 nt3 cv4 | generic co1 ci16",
        'n2_4-1_3x5x7_k211_s211_p000_o100_b1': "generic staps tl2 nt3 bias | generic taps tl4 nt3 cv1 | generic quads nt8 civ1",
        'n2_4-3_3x5x7_k211_s211_p000_o100_b1': "generic staps tl4 nt3 bias | generic gather tl4 vec0 | generic small",
        'n2_4-5_3x5x7_k211_s211_p000_o100_b1': "generic staps tl8 nt3 bias | generic gather tl4 vec0 | generic small",
        'n2_4-16_3x5x7_k211_s211_p000_o100_b1': "generic staps tl16 nt3 bias | generic taps tl4 nt3 cv4 | generic quads nt4 civ4",
        'n1_1-1_5x7x8_k311_s111_p100_o000_b1': "generic c1taps nt3 bias | generic c1taps nt3 | generic c1taps nt3",
        'n1_1-1_2x3x17_k411_s111_p000_o000_b1': "generic taps tl2 nt8 cv1 bias | generic taps tl2 nt6 cv1 | generic co1 ci1",
        'n1_1-3_2x3x17_k411_s111_p000_o000_b1': "generic taps tl4 nt8 cv1 bias | generic gather tl2 vec0 | generic small",
        'n1_1-5_2x3x17_k411_s111_p000_o000_b1': "generic taps tl8 nt8 cv1 bias | generic gather tl2 vec0 | generic small",
        'n1_1-16_2x3x17_k411_s111_p000_o000_b1': "generic taps tl16 nt8 cv1 bias | generic taps tl2 nt4 cv4 | generic co1 ci16",
        'n1_4-1_2x3x17_k411_s111_p000_o000_b1': "generic taps tl2 nt4 cv4 bias | generic taps tl4 nt6 cv1 | generic quads nt8 civ1",
        'n1_4-3_2x3x17_k411_s111_p000_o000_b1': "generic taps tl4 nt4 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-5_2x3x17_k411_s111_p000_o000_b1': "generic taps tl8 nt4 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-16_2x3x17_k411_s111_p000_o000_b1': "generic taps tl16 nt4 cv4 bias | generic taps tl4 nt4 cv4 | generic quads nt4 civ4",
        'n2_4-1_3x5x7_k511_s111_p200_o000_b1': "generic taps tl2 nt6 cv4 bias | generic taps tl4 nt6 cv1 | generic quads nt8 civ1",
        'n2_4-3_3x5x7_k511_s111_p200_o000_b1': "generic taps tl4 nt6 cv4 bias | generic gather tl4 vec0 | generic small",
        'n2_4-5_3x5x7_k511_s111_p200_o000_b1': "generic taps tl8 nt6 cv4 bias | generic gather tl4 vec0 | generic small",
        'n2_4-16_3x5x7_k511_s111_p200_o000_b1': "generic taps tl16 nt6 cv4 bias | generic taps tl4 nt6 cv4 | generic quads nt6 civ4",
        'n1_1-1_5x7x8_k511_s111_p200_o000_b1': "generic c1taps nt8 bias | generic c1taps nt8 | generic c1taps nt8",
        'n2_1-1_3x5x7_k333_s111_p111_o000_b1': "generic c1c1 bias | generic c1c1 | generic c1c1",
        'n2_4-1_3x5x7_k333_s111_p111_o000_b1': "generic gather tl2 vec1 bias | generic gather tl4 vec0 | cin1",
        'n2_4-3_3x5x7_k333_s111_p111_o000_b1': "generic gather tl4 vec1 bias | generic gather tl4 vec0 | generic lds",
        'n2_4-5_3x5x7_k333_s111_p111_o000_b1': "generic gather tl8 vec1 bias | generic gather tl4 vec0 | generic lds",
        'n2_4-16_3x5x7_k333_s111_p111_o000_b1': "generic gather tl16 vec1 bias | generic gather tl4 vec1 | wgrad6",
        'n1_4-1_4x6x8_k222_s111_p000_o000_b1': "generic taps tl2 nt8 cv4 bias | generic taps tl4 nt8 cv1 | generic quads nt8 civ1",
        'n1_4-3_4x6x8_k222_s111_p000_o000_b1': "generic taps tl4 nt8 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-5_4x6x8_k222_s111_p000_o000_b1': "generic taps tl8 nt8 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-16_4x6x8_k222_s111_p000_o000_b1': "generic taps tl16 nt8 cv4 bias | generic taps tl4 nt8 cv4 | generic quads nt8 civ4",
        'n1_4-1_3x4x5_k331_s221_p110_o000_b1': "generic staps tl2 nt4 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-3_3x4x5_k331_s221_p110_o000_b1': "generic staps tl4 nt4 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-5_3x4x5_k331_s221_p110_o000_b1': "generic staps tl8 nt4 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-16_3x4x5_k331_s221_p110_o000_b1': "generic staps tl16 nt4 bias | generic gather tl4 vec1 | generic lds",
        'n1_4-1_4x6x8_k333_s222_p111_o000_b1': "generic staps tl2 nt8 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-3_4x6x8_k333_s222_p111_o000_b1': "generic staps tl4 nt8 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-5_4x6x8_k333_s222_p111_o000_b1': "generic staps tl8 nt8 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-16_4x6x8_k333_s222_p111_o000_b1': "generic staps tl16 nt8 bias | generic gather tl4 vec1 | generic lds",
        'n1_4-1_4x6x8_k555_s222_p222_o000_b1': "generic strided tl2 vec1 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-3_4x6x8_k555_s222_p222_o000_b1': "generic strided tl4 vec1 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-5_4x6x8_k555_s222_p222_o000_b1': "generic strided tl8 vec1 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-16_4x6x8_k555_s222_p222_o000_b1': "generic strided tl16 vec1 bias | generic gather tl4 vec1 | generic lds",
        'n2_1-4_3x5x7_k111_s111_p000_o000_b1': "pointwise co2 bias | pointwise co2 | pointwise co2 vx4 dv0",
        'n2_3-4_3x5x7_k111_s111_p000_o000_b1': "pointwise co4 bias | pointwise co4 | pointwise co4 vx4 dv0",
        'n2_5-4_3x5x7_k111_s111_p000_o000_b1': "pointwise co8 bias | generic taps tl8 nt3 cv4 | pointwise co8 vx4 dv0",
        'n1_6-6_5x6x7_k222_s222_p000_o000_b1': "generic strided tl8 vec0 bias | generic gather tl8 vec0 | generic small",
        'n2_1-1_3x4x5_k444_s444_p000_o000_b1': "generic strided tl2 vec0 bias | generic gather tl2 vec0 | generic lds",
        'n1_8-4_5x5x6_k444_s222_p111_o000_b1': "generic staps tl4 nt8 bias | generic gather tl8 vec1 | generic lds",
        'n1_4-8_4x5x3_k333_s222_p111_o111_b1': "generic staps tl8 nt8 bias | generic gather tl4 vec1 | generic lds",
        'n1_8-8_3x4x5_k444_s444_p000_o000_b1': "generic staps tl8 nt3 bias | generic gather tl8 vec1 | generic lds",
        'n1_16-16_2x3x5_k444_s444_p000_o000_b1': "generic staps tl16 nt3 bias | generic gather tl16 vec1 | generic lds",
        'n1_1-1_3x5x7_k444_s444_p000_o000_b1': "generic strided tl2 vec0 bias | generic gather tl2 vec0 | generic lds",
        'n2_8-8_3x5x7_k444_s222_p111_o000_b1': "generic staps tl8 nt8 bias | generic gather tl8 vec1 | generic lds",
        'n2_4-8_3x5x7_k333_s222_p111_o111_b1': "generic staps tl8 nt8 bias | generic gather tl4 vec1 | generic lds",
        'n1_8-8_1x5x7_k222_s222_p000_o000_b0': "generic staps tl8 nt3 | generic taps tl8 nt8 cv4 | generic quads nt8 civ4",
    },
    ("TRANSPOSE", "bf16"): {
        'n1_1-1_2x3x17_k211_s111_p000_o000_b1': "generic taps tl2 nt3 cv1 bias | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n1_1-3_2x3x17_k211_s111_p000_o000_b1': "generic taps tl4 nt3 cv1 bias | generic gather tl2 vec0 | generic small",
        'n1_1-5_2x3x17_k211_s111_p000_o000_b1': "generic taps tl8 nt3 cv1 bias | generic gather tl2 vec0 | generic small",
        'n1_1-16_2x3x17_k211_s111_p000_o000_b1': "generic taps tl16 nt3 cv1 bias | generic taps tl2 nt3 cv4 | generic co1 ci16",
        'n1_2-1_2x3x17_k211_s111_p000_o000_b1': "generic gather tl2 vec0 bias | generic taps tl2 nt3 cv1 | generic small",
        'n1_2-3_2x3x17_k211_s111_p000_o000_b1': "generic gather tl4 vec0 bias | generic gather tl2 vec0 | generic small",
        'n1_2-5_2x3x17_k211_s111_p000_o000_b1': "generic gather tl8 vec0 bias | generic gather tl2 vec0 | generic small",
        'n1_2-16_2x3x17_k211_s111_p000_o000_b1': "generic gather tl16 vec0 bias | generic taps tl2 nt3 cv4 | generic small",
        'n1_4-1_2x3x17_k211_s111_p000_o000_b1': "generic taps tl2 nt3 cv4 bias | generic taps tl4 nt3 cv1 | generic quads nt8 civ1",
        'n1_4-3_2x3x17_k211_s111_p000_o000_b1': "generic taps tl4 nt3 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-5_2x3x17_k211_s111_p000_o000_b1': "generic taps tl8 nt3 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-16_2x3x17_k211_s111_p000_o000_b1': "generic taps tl16 nt3 cv4 bias | generic taps tl4 nt3 cv4 | generic quads nt4 civ4",
        'n2_1-1_3x5x7_k211_s211_p000_o100_b1': "generic strided tl2 vec0 bias | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n2_1-3_3x5x7_k211_s211_p000_o100_b1': "generic strided tl4 vec0 bias | generic gather tl2 vec0 | generic small",
        'n2_1-5_3x5x7_k211_s211_p000_o100_b1': "generic strided tl8 vec0 bias | generic gather tl2 vec0 | generic small",
        'n2_1-16_3x5x7_k211_s211_p000_o100_b1': "generic strided tl16 vec0 bias | generic taps tl2 nt3 cv4 | generic co1 ci16",
        'n2_4-1_3x5x7_k211_s211_p000_o100_b1': "generic staps tl2 nt3 bias | generic taps tl4 nt3 cv1 | generic quads nt8 civ1",
        'n2_4-3_3x5x7_k211_s211_p000_o100_b1': "generic staps tl4 nt3 bias | generic gather tl4 vec0 | generic small",
        'n2_4-5_3x5x7_k211_s211_p000_o100_b1': "generic staps tl8 nt3 bias | generic gather tl4 vec0 | generic small",
        'n2_4-16_3x5x7_k211_s211_p000_o100_b1': "generic staps tl16 nt3 bias | generic taps tl4 nt3 cv4 | generic quads nt4 civ4",
        'n1_1-1_5x7x8_k311_s111_p100_o000_b1': "generic taps tl2 nt3 cv1 bias | generic taps tl2 nt3 cv1 | generic co1 ci1",
        'n1_1-1_2x3x17_k411_s111_p000_o000_b1': "generic taps tl2 nt8 cv1 bias | generic taps tl2 nt6 cv1 | generic co1 ci1",
        'n1_1-3_2x3x17_k411_s111_p000_o000_b1': "generic taps tl4 nt8 cv1 bias | generic gather tl2 vec0 | generic small",
        'n1_1-5_2x3x17_k411_s111_p000_o000_b1': "generic taps tl8 nt8 cv1 bias | generic gather tl2 vec0 | generic small",
        'n1_1-16_2x3x17_k411_s111_p000_o000_b1': "generic taps tl16 nt8 cv1 bias | generic taps tl2 nt4 cv4 | generic co1 ci16",
        'n1_4-1_2x3x17_k411_s111_p000_o000_b1': "generic taps tl2 nt4 cv4 bias | generic taps tl4 nt6 cv1 | generic quads nt8 civ1",
        'n1_4-3_2x3x17_k411_s111_p000_o000_b1': "generic taps tl4 nt4 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-5_2x3x17_k411_s111_p000_o000_b1': "generic taps tl8 nt4 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-16_2x3x17_k411_s111_p000_o000_b1': "generic taps tl16 nt4 cv4 bias | generic taps tl4 nt4 cv4 | generic quads nt4 civ4",
        'n2_4-1_3x5x7_k511_s111_p200_o000_b1': "generic taps tl2 nt6 cv4 bias | generic taps tl4 nt6 cv1 | generic quads nt8 civ1",
        'n2_4-3_3x5x7_k511_s111_p200_o000_b1': "generic taps tl4 nt6 cv4 bias | generic gather tl4 vec0 | generic small",
        'n2_4-5_3x5x7_k511_s111_p200_o000_b1': "generic taps tl8 nt6 cv4 bias | generic gather tl4 vec0 | generic small",
        'n2_4-16_3x5x7_k511_s111_p200_o000_b1': "generic taps tl16 nt6 cv4 bias | generic taps tl4 nt6 cv4 | generic quads nt6 civ4",
        'n1_1-1_5x7x8_k511_s111_p200_o000_b1': "generic taps tl2 nt8 cv1 bias | generic taps tl2 nt6 cv1 | generic co1 ci1",
        'n2_1-1_3x5x7_k333_s111_p111_o000_b1': "generic c1c1 bias | generic c1c1 | generic c1c1",
        'n2_4-1_3x5x7_k333_s111_p111_o000_b1': "generic gather tl2 vec1 bias | generic gather tl4 vec0 | cin1",
        'n2_4-3_3x5x7_k333_s111_p111_o000_b1': "generic gather tl4 vec1 bias | generic gather tl4 vec0 | generic lds",
        'n2_4-5_3x5x7_k333_s111_p111_o000_b1': "generic gather tl8 vec1 bias | generic gather tl4 vec0 | generic lds",
        'n2_4-16_3x5x7_k333_s111_p111_o000_b1': "generic gather tl16 vec1 bias | generic gather tl4 vec1 | wgrad4",
        'n1_4-1_4x6x8_k222_s111_p000_o000_b1': "generic taps tl2 nt8 cv4 bias | generic taps tl4 nt8 cv1 | generic quads nt8 civ1",
        'n1_4-3_4x6x8_k222_s111_p000_o000_b1': "generic taps tl4 nt8 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-5_4x6x8_k222_s111_p000_o000_b1': "generic taps tl8 nt8 cv4 bias | generic gather tl4 vec0 | generic small",
        'n1_4-16_4x6x8_k222_s111_p000_o000_b1': "generic taps tl16 nt8 cv4 bias | generic taps tl4 nt8 cv4 | generic quads nt8 civ4",
        'n1_4-1_3x4x5_k331_s221_p110_o000_b1': "generic staps tl2 nt4 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-3_3x4x5_k331_s221_p110_o000_b1': "generic staps tl4 nt4 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-5_3x4x5_k331_s221_p110_o000_b1': "generic staps tl8 nt4 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-16_3x4x5_k331_s221_p110_o000_b1': "generic staps tl16 nt4 bias | generic gather tl4 vec1 | generic lds",
        'n1_4-1_4x6x8_k333_s222_p111_o000_b1': "generic staps tl2 nt8 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-3_4x6x8_k333_s222_p111_o000_b1': "generic staps tl4 nt8 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-5_4x6x8_k333_s222_p111_o000_b1': "generic staps tl8 nt8 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-16_4x6x8_k333_s222_p111_o000_b1': "generic staps tl16 nt8 bias | generic gather tl4 vec1 | generic lds",
        'n1_4-1_4x6x8_k555_s222_p222_o000_b1': "generic strided tl2 vec1 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-3_4x6x8_k555_s222_p222_o000_b1': "generic strided tl4 vec1 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-5_4x6x8_k555_s222_p222_o000_b1': "generic strided tl8 vec1 bias | generic gather tl4 vec0 | generic lds",
        'n1_4-16_4x6x8_k555_s222_p222_o000_b1': "generic strided tl16 vec1 bias | generic gather tl4 vec1 | generic lds",
        'n2_1-4_3x5x7_k111_s111_p000_o000_b1': "pointwise co2 bias | pointwise co2 | pointwise co2 vx4 dv0",
        'n2_3-4_3x5x7_k111_s111_p000_o000_b1': "pointwise co4 bias | pointwise co4 | pointwise co4 vx4 dv0",
        'n2_5-4_3x5x7_k111_s111_p000_o000_b1': "pointwise co8 bias | generic taps tl8 nt3 cv4 | pointwise co8 vx4 dv0",
        'n1_6-6_5x6x7_k222_s222_p000_o000_b1': "generic strided tl8 vec0 bias | generic gather tl8 vec0 | generic small",
        'n2_1-1_3x4x5_k444_s444_p000_o000_b1': "generic strided tl2 vec0 bias | generic gather tl2 vec0 | generic lds",
        'n1_8-4_5x5x6_k444_s222_p111_o000_b1': "generic staps tl4 nt8 bias | generic gather tl8 vec1 | generic lds",
        'n1_4-8_4x5x3_k333_s222_p111_o111_b1': "generic staps tl8 nt8 bias | generic gather tl4 vec1 | generic lds",
        'n1_8-8_3x4x5_k444_s444_p000_o000_b1': "generic staps tl8 nt3 bias | generic gather tl8 vec1 | generic lds",
        'n1_16-16_2x3x5_k444_s444_p000_o000_b1': "generic staps tl16 nt3 bias | generic gather tl16 vec1 | generic lds",
        'n1_1-1_3x5x7_k444_s444_p000_o000_b1': "generic strided tl2 vec0 bias | generic gather tl2 vec0 | generic lds",
        'n2_8-8_3x5x7_k444_s222_p111_o000_b1': "generic staps tl8 nt8 bias | generic gather tl8 vec1 | generic lds",
        'n2_4-8_3x5x7_k333_s222_p111_o111_b1': "generic staps tl8 nt8 bias | generic gather tl4 vec1 | generic lds",
        'n1_8-8_1x5x7_k222_s222_p000_o000_b0': "generic staps tl8 nt3 | generic taps tl8 nt8 cv4 | generic quads nt8 civ4",
    },
    ("WS_WGRAD", "f32"): {
        'wgrad_c1c1': "generic c1c1 | generic c1c1 | generic c1c1",
        'wgrad_c1taps': "generic c1taps nt3 | generic c1taps nt3 | generic c1taps nt3",
        'wgrad_cin1': "generic cin1 co8 | generic gather tl2 vec1 | generic cin1 co8",
        'wgrad_co1': "generic taps tl2 nt3 cv4 | generic taps tl8 nt3 cv1 | generic co1 ci8",
        'wgrad_quads': "generic taps tl8 nt3 cv4 | generic taps tl8 nt3 cv4 | generic quads nt4 civ4",
        'wgrad_quads_dy_misaligned': "generic taps tl8 nt3 cv4 | generic gather tl8 vec0 | generic small",
        'wgrad_small': "generic gather tl8 vec0 | generic gather tl4 vec0 | generic small",
        'wgrad_lds': "generic gather tl8 vec0 | generic gather tl4 vec0 | generic lds",
        'wgrad_pointwise': "pointwise co2 | pointwise co2 | pointwise co2 vx4 dv1",
    },
    ("WS_WGRAD", "bf16"): {
        'wgrad_cin1_bf16': "generic cin1 co16 | generic gather tl2 vec1 | generic cin1 co16",
        'wgrad_quads_bf16': "generic taps tl16 nt6 cv4 | generic staps tl8 nt3 | generic quads nt6 civ4",
        'wgrad_pointwise_bf16': "pointwise co4 | pointwise co4 | pointwise co4 vx8 dv1",
    },
})
