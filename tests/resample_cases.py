"""The pool and upsample parity cases of tests/test_ops_gpu.py and tests/test_bf16_gpu.py as named rows (data only), each with the
kernel it declares for its forward and its backward pass: the names of mri3d_maxpool3d_route / mri3d_upsample3d_route
(include/mri3d.h).  tests/test_resample_routes.py checks, without a GPU, that every row reaches what it declares and that no name
is left without a row.  Every case runs with batch size N; tensors are fresh allocations unless a row says otherwise.  The second
half of the file holds the rows of the float64 parity net (tests/test_resample_parity_gpu.py), which also declare plan numbers."""
import collections

N = 2

# MaxPool3d(k, s) of a (N, c, *sp) tensor
PoolRow = collections.namedtuple("PoolRow", "id dtype c sp k s fwd bwd")
# max_pool3d_skip(x, 2): dskip arrives as the last c channels of a buffer `pad` channels wider; fwd / bwd are {dtype: name}.  The
# backward sums both gradients in every run of the test: where only one output is used, autograd hands over dense zeros for the other.
SkipRow = collections.namedtuple("SkipRow", "id c sp pad fwd bwd")
# upsample3d(x, size=size, scale_factor=scale, mode=mode, align_corners=ac) of a (N, c, *sp) tensor
UpRow = collections.namedtuple("UpRow", "id dtype mode size scale ac c sp fwd bwd")

# tests/test_ops_gpu.py::test_max_pool3d
POOL = [
    PoolRow("c16_even", "f32", 16, (8, 12, 10), 2, 2, "maxpool2_fwd<f32,4>", "maxpool_bwd<f32,4>"),
    PoolRow("c8_odd", "f32", 8, (9, 7, 11), 2, 2, "maxpool_fwd<f32,4>", "maxpool_bwd<f32,4>"),
    PoolRow("c3", "f32", 3, (6, 6, 6), 2, 2, "maxpool_fwd<f32,1>", "maxpool_bwd<f32,1>"),
    PoolRow("c4_k4s2", "f32", 4, (13, 12, 14), 4, 2, "maxpool_fwd<f32,4>", "maxpool_bwd<f32,4>"),
    PoolRow("c1", "f32", 1, (8, 8, 8), 2, 2, "maxpool_fwd<f32,1>", "maxpool_bwd<f32,1>"),
    PoolRow("c64_even", "f32", 64, (4, 6, 4), 2, 2, "maxpool2_fwd<f32,4>", "maxpool_bwd<f32,4>"),
]


def _both(fmt, f32, bf16):
    return {"f32": fmt % ("f32", f32), "bf16": fmt % ("bf16", bf16)}


# tests/test_ops_gpu.py::test_max_pool3d_skip_sums_both_gradients_in_the_pool_kernel
POOL_SKIP = [
    SkipRow("c16_even", 16, (6, 8, 10), 0, _both("maxpool2_fwd<%s,%d>", 4, 8), _both("maxpool_bwd<%s,%d>+add", 4, 8)),
    SkipRow("c8_odd_pitched", 8, (5, 7, 9), 8, _both("maxpool_fwd<%s,%d>", 4, 8), _both("maxpool_bwd<%s,%d>+add", 4, 8)),
    SkipRow("c3", 3, (4, 4, 6), 0, _both("maxpool_fwd<%s,%d>", 1, 1), _both("maxpool_bwd<%s,%d>+add", 1, 1)),
    SkipRow("c32_one_window_pitched", 32, (2, 2, 2), 16, _both("maxpool2_fwd<%s,%d>", 4, 8), _both("maxpool_bwd<%s,%d>+add", 4, 8)),
]

_TILE, _MARCH = "upsample2x_bwd<%s>", "upsample2x_bwd_march<%s>"

# tests/test_ops_gpu.py::test_upsample3d
UP = [
    UpRow("nearest_x2", "f32", "nearest", None, 2, None, 16, (5, 6, 7), "upsample_fwd<f32,4>", "upsample_nearest_int_bwd<f32,2>"),
    UpRow("nearest_x4", "f32", "nearest", None, 4, None, 8, (3, 4, 2), "upsample_fwd<f32,4>", "upsample_nearest_int_bwd<f32,4>"),
    UpRow("nearest_size", "f32", "nearest", (9, 11, 13), None, None, 4, (4, 5, 6), "upsample_fwd<f32,4>", "tables+upsample_bwd<f32,4>"),
    UpRow("nearest_size_c1", "f32", "nearest", (7, 7, 7), None, None, 1, (7, 3, 9), "upsample_fwd<f32,1>", "tables+upsample_bwd<f32,1>"),
    UpRow("trilinear_x2_c32", "f32", "trilinear", None, 2, False, 32, (5, 6, 4), "upsample2x_fwd_march<f32,4,8>", _MARCH % "f32"),
    UpRow("trilinear_x2_corners", "f32", "trilinear", None, 2, True, 8, (5, 6, 4), "upsample_fwd<f32,4>", "tables+upsample_bwd<f32,4>"),
    UpRow("trilinear_size", "f32", "trilinear", (7, 9, 11), None, False, 4, (4, 5, 6), "upsample_fwd<f32,4>", "tables+upsample_bwd<f32,4>"),
    UpRow("trilinear_x2_c3", "f32", "trilinear", None, 2, False, 3, (1, 4, 5), "upsample_fwd<f32,1>", "tables+upsample_bwd<f32,1>"),
    # x2 trilinear marching along D (4 x 16 coarse columns, 16-plane segments): ragged columns in h and w, two segments,
    # 8 / 4 / 2 / 1 pieces per voxel, a half-empty second channel pass (24 channels), two full passes (64)
    UpRow("march_c64", "f32", "trilinear", None, 2, False, 64, (18, 9, 19), "upsample2x_fwd_march<f32,4,8>", _MARCH % "f32"),
    UpRow("march_c24", "f32", "trilinear", None, 2, False, 24, (3, 5, 33), "upsample2x_fwd_march<f32,4,4>", _TILE % "f32"),
    UpRow("march_c16", "f32", "trilinear", None, 2, False, 16, (17, 4, 16), "upsample2x_fwd_march<f32,4,4>", _MARCH % "f32"),
    UpRow("march_c8", "f32", "trilinear", None, 2, False, 8, (2, 7, 5), "upsample2x_fwd_march<f32,4,2>", _TILE % "f32"),
    UpRow("march_c4_long", "f32", "trilinear", None, 2, False, 4, (33, 3, 18), "upsample2x_fwd_march<f32,4,1>", _TILE % "f32"),
    UpRow("march_c4_one_plane", "f32", "trilinear", None, 2, False, 4, (1, 3, 5), "upsample2x_fwd_march<f32,4,1>", _TILE % "f32"),
    UpRow("march_c8_one_row", "f32", "trilinear", None, 2, False, 8, (2, 1, 1), "upsample2x_fwd_march<f32,4,2>", _TILE % "f32"),
    UpRow("march_c12", "f32", "trilinear", None, 2, False, 12, (5, 1, 21), "upsample2x_fwd_march<f32,4,2>", _TILE % "f32"),
]

# tests/test_bf16_gpu.py::test_pool_upsample_cat_add_bf16: the pool, then a trilinear and a nearest x2 upsample of the pooled tensor
BF16_CHAIN_POOL = PoolRow("chain_pool", "bf16", 8, (8, 10, 12), 2, 2, "maxpool2_fwd<bf16,8>", "maxpool_bwd<bf16,8>")
BF16_CHAIN_UP = [
    UpRow("chain_trilinear", "bf16", "trilinear", None, 2, False, 8, (4, 5, 6), "upsample2x_fwd_march<bf16,8,1>", _TILE % "bf16"),
    UpRow("chain_nearest", "bf16", "nearest", None, 2, None, 8, (4, 5, 6), "upsample_fwd<bf16,4>", "upsample_nearest_int_bwd<bf16,2>"),
]

# tests/test_bf16_gpu.py::test_trilinear_x2_forward_backward_bf16
BF16_TRILINEAR = [
    UpRow("bf16_c8", "bf16", "trilinear", None, 2, False, 8, (5, 9, 19), "upsample2x_fwd_march<bf16,8,1>", _TILE % "bf16"),
    UpRow("bf16_c16", "bf16", "trilinear", None, 2, False, 16, (17, 4, 16), "upsample2x_fwd_march<bf16,8,2>", _MARCH % "bf16"),
    UpRow("bf16_c32", "bf16", "trilinear", None, 2, False, 32, (3, 6, 33), "upsample2x_fwd_march<bf16,8,4>", _MARCH % "bf16"),
    UpRow("bf16_c64", "bf16", "trilinear", None, 2, False, 64, (18, 5, 7), "upsample2x_fwd_march<bf16,8,8>", _MARCH % "bf16"),
    UpRow("bf16_c12", "bf16", "trilinear", None, 2, False, 12, (4, 5, 18), "upsample2x_fwd_march<bf16,4,2>", _TILE % "bf16"),
    UpRow("bf16_c40", "bf16", "trilinear", None, 2, False, 40, (2, 9, 17), "upsample2x_fwd_march<bf16,8,4>", _TILE % "bf16"),
]

# tests/test_bf16_gpu.py::test_nearest_upsampling_backward_with_an_integer_scale_bf16
BF16_NEAREST = [
    UpRow("bf16_nearest_x2", "bf16", "nearest", None, 2, None, 8, (3, 5, 7), "upsample_fwd<bf16,4>", "upsample_nearest_int_bwd<bf16,2>"),
    UpRow("bf16_nearest_x4", "bf16", "nearest", None, 4, None, 8, (3, 5, 7), "upsample_fwd<bf16,4>", "upsample_nearest_int_bwd<bf16,4>"),
]

POOL_ROWS = POOL + [BF16_CHAIN_POOL]
UP_ROWS = UP + BF16_CHAIN_UP + BF16_TRILINEAR + BF16_NEAREST


# ================================================================================================ float64 parity rows
# tests/test_resample_parity_gpu.py runs every row below (and every row above) against tests/resample_ref.py; DESIGN §4.8 has
# the table of plan corners and the rows that reach them.  A row runs in every storage type of `dtypes`.
#   layout   {tensor: (width, off)}: the tensor is the channels [off, off + c) of a `width`-channel NDHWC buffer inside guard bands
#            (x; out: upsample3d(out=(buf, off)); dy; dskip).  Tensors not named are fresh dense allocations.
#   fwd, bwd the kernel names, {dtype: name}
#   nums     {"fwd" | "bwd": {field of ops.pool_plan / ops.upsample_plan: value or {dtype: value}}}: the numbers the row is there for
#   values   how the pool's input is drawn: normal | ties (eight distinct values) | neginf (whole windows of -inf) | nan
#            (scattered) | negative (everything below -1: padding must not win)
ParityPool = collections.namedtuple("ParityPool", "id c sp k s p addend values dtypes layout fwd bwd nums")
ParityUp = collections.namedtuple("ParityUp", "id mode size scale ac c sp dtypes layout fwd bwd nums")
BOTH = ("f32", "bf16")


def _t3(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3


def _pool(id, c, sp, k=2, s=2, p=0, addend=False, values="normal", dtypes=BOTH, layout=None, fwd=None, bwd=None, nums=None):
    """fwd: (kernel, vec f32, vec bf16); bwd: (vec f32, vec bf16)"""
    add = "+add" if addend else ""
    return ParityPool(id, c, tuple(sp), _t3(k), _t3(s), _t3(p), addend, values, dtypes, layout or {},
                      {"f32": "%s<f32,%d>" % (fwd[0], fwd[1]), "bf16": "%s<bf16,%d>" % (fwd[0], fwd[2])},
                      {"f32": "maxpool_bwd<f32,%d>%s" % (bwd[0], add), "bf16": "maxpool_bwd<bf16,%d>%s" % (bwd[1], add)}, nums or {})


def _with_and_without_addend(*a, **kw):
    return [_pool(a[0], *a[1:], **kw), _pool(a[0] + "_add", *a[1:], addend=True, **kw)]


def _up(id, mode, c, sp, size=None, scale=None, ac=None, dtypes=BOTH, layout=None, fwd=None, bwd=None, nums=None):
    """fwd / bwd: a name with %s for the storage type, or (f32 name, bf16 name) with %s likewise"""
    def names(v):
        f, b = (v, v) if isinstance(v, str) else v
        return {"f32": f % "f32", "bf16": b % "bf16"}
    return ParityUp(id, mode, size, scale, ac, c, tuple(sp), dtypes, layout or {}, names(fwd), names(bwd), nums or {})


_SLAB1, _SLAB4 = "upsample_fwd<%s,1>", "upsample_fwd<%s,4>"
_TAB1, _TAB4 = "tables+upsample_bwd<%s,1>", "tables+upsample_bwd<%s,4>"
_FM = "upsample2x_fwd_march<%%s,%d,%d>"

# ---- the instantiations no earlier row launched (bf16 channels in quads but not octets, odd bf16 channels)
PARITY_POOL_UNREACHED = (
    _with_and_without_addend("c4_even", 4, (4, 6, 8), fwd=("maxpool2_fwd", 4, 4), bwd=(4, 4)) +
    [_pool("c12_odd_extents", 12, (5, 7, 9), fwd=("maxpool_fwd", 4, 4), bwd=(4, 4)),
     _pool("c3_no_addend", 3, (4, 6, 6), fwd=("maxpool_fwd", 1, 1), bwd=(1, 1))])
PARITY_UP_UNREACHED = [
    _up("x2_c4", "trilinear", 4, (3, 5, 17), scale=2, ac=False, fwd=_FM % (4, 1), bwd=_TILE, nums={"fwd": {"passes": 1}}),
    _up("x2_c20_two_passes", "trilinear", 20, (5, 3, 6), scale=2, ac=False, fwd=_FM % (4, 4), bwd=_TILE, nums={"fwd": {"passes": 2}}),
    _up("x2_c36_one_live_piece", "trilinear", 36, (3, 5, 4), scale=2, ac=False, fwd=_FM % (4, 8), bwd=_TILE, nums={"fwd": {"passes": 2}}),
    _up("x2_c3", "trilinear", 3, (3, 4, 5), scale=2, ac=False, fwd=_SLAB1, bwd=_TAB1),
    _up("size_c4", "trilinear", 4, (4, 5, 6), size=(7, 9, 11), ac=False, fwd=_SLAB4, bwd=_TAB4),
]

# ---- alignment and pitch through the public API: 8-byte aligned bf16 (quads instead of octets), 4- and 8-byte aligned f32 (no vector)
_BF8 = {"x": (24, 4), "out": (24, 4), "dy": (24, 4), "dskip": (24, 4)}
PARITY_POOL_ALIGN = [
    _pool("bf16_c16_at_4_of_24", 16, (4, 6, 8), dtypes=("bf16",), layout=_BF8, fwd=("maxpool2_fwd", 4, 4), bwd=(4, 4)),
    _pool("bf16_c16_at_4_of_24_add", 16, (4, 6, 8), addend=True, dtypes=("bf16",), layout=_BF8, fwd=("maxpool2_fwd", 4, 4), bwd=(4, 4)),
    _pool("f32_c8_at_1_of_12", 8, (4, 6, 8), dtypes=("f32",), layout={"x": (12, 1), "dy": (12, 1)}, fwd=("maxpool_fwd", 1, 1), bwd=(1, 1)),
    _pool("f32_c8_at_2_of_12_add", 8, (5, 6, 7), addend=True, dtypes=("f32",), layout={"x": (12, 2), "dy": (12, 2), "dskip": (12, 2)},
          fwd=("maxpool_fwd", 1, 1), bwd=(1, 1)),
]
PARITY_UP_ALIGN = [
    _up("bf16_x2_c16_at_4_of_24", "trilinear", 16, (9, 5, 17), scale=2, ac=False, dtypes=("bf16",), layout=_BF8, fwd=_FM % (4, 4),
        bwd=_MARCH, nums={"fwd": {"vec": 4}, "bwd": {"vec": 4}}),
    _up("f32_x2_c8_at_2_of_12", "trilinear", 8, (3, 5, 6), scale=2, ac=False, dtypes=("f32",), layout={"x": (12, 2), "out": (12, 2), "dy": (12, 2)},
        fwd=_SLAB1, bwd=_TAB1),
    _up("f32_nearest_x2_c8_at_1_of_12", "nearest", 8, (3, 5, 6), scale=2, dtypes=("f32",), layout={"x": (12, 1), "out": (12, 1), "dy": (12, 1)},
        fwd=_SLAB1, bwd=_TAB1),
]

# ---- segment lengths of the x2 forward (the rows above this section all run segl = 4), and the backward of the same shapes
PARITY_UP_SEGMENTS = [
    _up("x2_c20_segl16", "trilinear", 20, (2045, 5, 3), scale=2, ac=False, fwd=_FM % (4, 4), bwd=_TILE,
        nums={"fwd": {"segl": 16, "segs": 128, "passes": 2, "tiles_h": 2, "items": 1024}, "bwd": {"items": 4092, "grid": 2048}}),
    _up("x2_c20_segl8", "trilinear", 20, (1030, 5, 3), scale=2, ac=False, fwd=_FM % (4, 4), bwd=_TILE,
        nums={"fwd": {"segl": 8, "segs": 129, "passes": 2, "tiles_h": 2, "items": 1032}, "bwd": {"items": 2060, "grid": 2048}}),
    _up("x2_c24_segl8_octets", "trilinear", 24, (1030, 5, 3), scale=2, ac=False, fwd=(_FM % (4, 4), _FM % (8, 2)), bwd=_TILE,
        nums={"fwd": {"segl": 8, "segs": 129, "passes": 2, "vec": {"f32": 4, "bf16": 8}}}),
]

# ---- more items (slabs) than workgroups: the second iteration of every grid-stride loop, the XCD remap with items % 8 != 0
PARITY_UP_LOOPS = [
    _up("x2_c4_8194_items", "trilinear", 4, (65552, 1, 1), scale=2, ac=False, dtypes=("f32",), fwd=_FM % (4, 1), bwd=_TILE,
        nums={"fwd": {"items": 8194, "grid": 8192, "segl": 16}}),
    _up("x2_c8_8194_items", "trilinear", 8, (65552, 1, 1), scale=2, ac=False, dtypes=("bf16",), fwd=_FM % (8, 1), bwd=_TILE,
        nums={"fwd": {"items": 8194, "grid": 8192, "segl": 16}}),
    _up("x2_c20_8196_items", "trilinear", 20, (32784, 1, 1), scale=2, ac=False, fwd=_FM % (4, 4), bwd=_TILE,
        nums={"fwd": {"items": 8196, "grid": 8192, "passes": 2}}),
    _up("x2_c16_bwd_6148_items", "trilinear", 16, (12296, 1, 17), scale=2, ac=False, fwd=(_FM % (4, 4), _FM % (8, 2)), bwd=_MARCH,
        nums={"bwd": {"items": 6148, "grid": 6144}}),
    _up("x2_c12_bwd_2052_items", "trilinear", 12, (1026, 5, 1), scale=2, ac=False, fwd=_FM % (4, 2), bwd=_TILE,
        nums={"bwd": {"items": 2052, "grid": 2048}}),
]
_NI = "upsample_nearest_int_bwd<%%s,%d>"
for _c, _f, _b in ((1, _SLAB1, _TAB1), (4, _SLAB4, _TAB4)):
    _g = {"fwd": {"grid": 8192}, "bwd": {"grid": 8192}}
    PARITY_UP_LOOPS += [
        _up("slab_nearest_x2_c%d" % _c, "nearest", _c, (4200, 1, 2), scale=2, fwd=_f, bwd=_b if _c == 1 else _NI % 2, nums=_g),
        _up("slab_nearest_x4_c%d" % _c, "nearest", _c, (4200, 1, 2), scale=4, fwd=_f, bwd=_b if _c == 1 else _NI % 4, nums=_g),
        _up("slab_nearest_size_c%d" % _c, "nearest", _c, (4200, 1, 2), size=(4301, 3, 5), fwd=_f, bwd=_b, nums=_g),
        _up("slab_trilinear_size_c%d" % _c, "trilinear", _c, (4200, 1, 2), size=(4301, 3, 5), ac=False, fwd=_f, bwd=_b, nums=_g),
    ]
PARITY_POOL_LOOPS = (
    _with_and_without_addend("loop_c1", 1, (8200, 2, 2), fwd=("maxpool_fwd", 1, 1), bwd=(1, 1), nums={"fwd": {"grid": 8192}, "bwd": {"grid": 8192}}) +
    _with_and_without_addend("loop_c4", 4, (8200, 2, 2), fwd=("maxpool2_fwd", 4, 4), bwd=(4, 4), nums={"fwd": {"grid": 8192}, "bwd": {"grid": 8192}}) +
    [_pool("loop_c8", 8, (8200, 2, 2), fwd=("maxpool2_fwd", 4, 8), bwd=(4, 8), nums={"fwd": {"grid": 8192}, "bwd": {"grid": 8192}}),
     _pool("loop_c8_odd_w", 8, (8200, 2, 3), fwd=("maxpool_fwd", 4, 8), bwd=(4, 8), nums={"fwd": {"grid": 8192}, "bwd": {"grid": 8192}})])

# ---- slabs that are a part of a plane (hch < the H extent of the pass), the last part ragged
PARITY_POOL_CHUNKS = [
    _pool("chunks_c16_even", 16, (2, 26, 80), fwd=("maxpool2_fwd", 4, 8), bwd=(4, 8),
          nums={"fwd": {"hch": {"f32": 6, "bf16": 12}}, "bwd": {"hch": {"f32": 6, "bf16": 12}}}),
    _pool("chunks_c16_odd_w", 16, (2, 26, 81), fwd=("maxpool_fwd", 4, 8), bwd=(4, 8),
          nums={"fwd": {"hch": {"f32": 12, "bf16": 13}}, "bwd": {"hch": {"f32": 6, "bf16": 12}}}),
    _pool("chunks_c32_odd_w", 32, (2, 26, 81), fwd=("maxpool_fwd", 4, 8), bwd=(4, 8),
          nums={"fwd": {"hch": {"f32": 6, "bf16": 12}}, "bwd": {"hch": {"f32": 3, "bf16": 6}}}),
]
PARITY_POOL_CHUNKS.append(_pool("chunks_c3", 3, (2, 14, 300), fwd=("maxpool_fwd", 1, 1), bwd=(1, 1), nums={"fwd": {"hch": 4}, "bwd": {"hch": 2}}))
PARITY_UP_CHUNKS = [
    _up("chunks_nearest_size_c3", "nearest", 3, (2, 9, 300), size=(3, 19, 601), fwd=_SLAB1, bwd=_TAB1, nums={"fwd": {"hch": 1}, "bwd": {"hch": 2}}),
    _up("chunks_trilinear_size_c3", "trilinear", 3, (2, 9, 300), size=(3, 19, 601), ac=False, fwd=_SLAB1, bwd=_TAB1,
        nums={"fwd": {"hch": 1}, "bwd": {"hch": 2}}),
    # slabs that are parts of a plane AND more of them than workgroups: 2 x 2050 planes of 2 rows of 1026 elements
    _up("chunks_and_loop_nearest_c1", "nearest", 1, (1025, 1, 513), scale=2, fwd=_SLAB1, bwd=_TAB1, nums={"fwd": {"hch": 1, "grid": 8192}}),
    _up("chunks_nearest_x2", "nearest", 16, (2, 9, 70), scale=2, fwd=_SLAB4, bwd=_NI % 2, nums={"fwd": {"hch": 3}, "bwd": {"hch": 7}}),
    _up("chunks_nearest_size", "nearest", 16, (2, 9, 70), size=(3, 19, 141), fwd=_SLAB4, bwd=_TAB4, nums={"fwd": {"hch": 3}, "bwd": {"hch": 7}}),
    _up("chunks_trilinear_size", "trilinear", 16, (2, 9, 70), size=(3, 19, 141), ac=False, fwd=_SLAB4, bwd=_TAB4,
        nums={"fwd": {"hch": 3}, "bwd": {"hch": 7}}),
]

# ---- pool geometries: padding, anisotropic windows, gaps between windows (stride > kernel), tap index 255, k4 s2 p2
PARITY_POOL_GEOMETRY = (
    _with_and_without_addend("k3s2p1", 8, (7, 9, 11), k=3, s=2, p=1, fwd=("maxpool_fwd", 4, 8), bwd=(4, 8)) +
    _with_and_without_addend("k122", 4, (3, 6, 8), k=(1, 2, 2), s=(1, 2, 2), fwd=("maxpool_fwd", 4, 4), bwd=(4, 4)) +
    _with_and_without_addend("k2s3_gaps", 8, (8, 9, 10), k=2, s=3, fwd=("maxpool_fwd", 4, 8), bwd=(4, 8)) +
    _with_and_without_addend("k488_tap255", 4, (8, 16, 16), k=(4, 8, 8), s=(4, 8, 8), fwd=("maxpool_fwd", 4, 4), bwd=(4, 4)) +
    _with_and_without_addend("k4s2p2", 8, (9, 8, 7), k=4, s=2, p=2, fwd=("maxpool_fwd", 4, 8), bwd=(4, 8)))

# ---- values: ties in most windows, whole windows of -inf, scattered NaN, all-negative inputs under padding
PARITY_POOL_VALUES = [
    _pool("ties_k2", 8, (8, 10, 12), values="ties", fwd=("maxpool2_fwd", 4, 8), bwd=(4, 8)),
    _pool("ties_k3s2p1", 8, (7, 9, 11), k=3, s=2, p=1, values="ties", fwd=("maxpool_fwd", 4, 8), bwd=(4, 8)),
    _pool("ties_k4s2_c3", 3, (9, 8, 10), k=4, s=2, values="ties", fwd=("maxpool_fwd", 1, 1), bwd=(1, 1)),
    _pool("neginf_k2", 8, (8, 10, 12), values="neginf", fwd=("maxpool2_fwd", 4, 8), bwd=(4, 8)),
    _pool("neginf_k3s2p1", 4, (7, 9, 11), k=3, s=2, p=1, values="neginf", fwd=("maxpool_fwd", 4, 4), bwd=(4, 4)),
    _pool("nan_k2", 8, (8, 10, 12), values="nan", fwd=("maxpool2_fwd", 4, 8), bwd=(4, 8)),
    _pool("nan_k3s2p1_add", 4, (7, 9, 11), k=3, s=2, p=1, addend=True, values="nan", fwd=("maxpool_fwd", 4, 4), bwd=(4, 4)),
    _pool("negative_k3s2p1", 8, (7, 9, 11), k=3, s=2, p=1, values="negative", fwd=("maxpool_fwd", 4, 8), bwd=(4, 8)),
    _pool("negative_k4s2p2", 3, (9, 8, 7), k=4, s=2, p=2, values="negative", fwd=("maxpool_fwd", 1, 1), bwd=(1, 1)),
]

# ---- coordinates: a scale of 1.5, down-sizing, output and input extents of 1, corners (extents above 256: the slab_* rows)
PARITY_UP_COORDS = [
    _up("trilinear_x1_5", "trilinear", 4, (4, 5, 6), scale=1.5, ac=False, fwd=_SLAB4, bwd=_TAB4),
    _up("nearest_x1_5", "nearest", 4, (4, 5, 6), scale=1.5, fwd=_SLAB4, bwd=_TAB4),
    _up("trilinear_down", "trilinear", 8, (9, 11, 13), size=(4, 5, 6), ac=False, fwd=_SLAB4, bwd=_TAB4),
    _up("trilinear_down_corners", "trilinear", 3, (9, 11, 13), size=(4, 5, 6), ac=True, fwd=_SLAB1, bwd=_TAB1),
    _up("trilinear_out1", "trilinear", 4, (5, 6, 7), size=(1, 9, 1), ac=False, fwd=_SLAB4, bwd=_TAB4),
    _up("trilinear_out1_corners", "trilinear", 4, (5, 6, 7), size=(1, 9, 1), ac=True, fwd=_SLAB4, bwd=_TAB4),
    _up("trilinear_in1", "trilinear", 4, (1, 6, 1), size=(3, 9, 4), ac=False, fwd=_SLAB4, bwd=_TAB4),
    _up("trilinear_in1_corners", "trilinear", 4, (1, 6, 1), size=(3, 9, 4), ac=True, fwd=_SLAB4, bwd=_TAB4),
    _up("nearest_in1", "nearest", 4, (1, 6, 1), size=(3, 9, 4), fwd=_SLAB4, bwd=_TAB4),
    _up("trilinear_corners_300", "trilinear", 4, (300, 2, 3), size=(701, 3, 5), ac=True, fwd=_SLAB4, bwd=_TAB4),
]


def _old_pool(r):
    return ParityPool("old_" + r.id, r.c, r.sp, _t3(r.k), _t3(r.s), (0, 0, 0), False, "normal", (r.dtype,), {}, {r.dtype: r.fwd}, {r.dtype: r.bwd}, {})


def _old_skip(r):
    layout = {"dskip": (r.c + r.pad, r.pad)} if r.pad else {}
    return ParityPool("old_skip_" + r.id, r.c, r.sp, (2, 2, 2), (2, 2, 2), (0, 0, 0), True, "normal", BOTH, layout, r.fwd, r.bwd, {})


def _old_up(r):
    nums = {"fwd": {"segl": 4}} if r.fwd.startswith("upsample2x_fwd_march") else {}
    return ParityUp("old_" + r.id, r.mode, r.size, r.scale, r.ac, r.c, r.sp, (r.dtype,), {}, {r.dtype: r.fwd}, {r.dtype: r.bwd}, nums)


PARITY_POOL = ([_old_pool(r) for r in POOL_ROWS] + [_old_skip(r) for r in POOL_SKIP] + PARITY_POOL_UNREACHED + PARITY_POOL_ALIGN +
               PARITY_POOL_LOOPS + PARITY_POOL_CHUNKS + PARITY_POOL_GEOMETRY + PARITY_POOL_VALUES)
PARITY_UP = ([_old_up(r) for r in UP_ROWS] + PARITY_UP_UNREACHED + PARITY_UP_ALIGN + PARITY_UP_SEGMENTS + PARITY_UP_LOOPS +
             PARITY_UP_CHUNKS + PARITY_UP_COORDS)
PARITY_PAIRS = [(r, t) for r in PARITY_POOL + PARITY_UP for t in r.dtypes]
PARITY_IDS = ["%s-%s-%s" % ("pool" if isinstance(r, ParityPool) else "up", r.id, t) for r, t in PARITY_PAIRS]
assert len(set(PARITY_IDS)) == len(PARITY_IDS)
