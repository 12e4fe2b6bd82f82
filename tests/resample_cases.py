"""The pool and upsample parity cases of tests/test_ops_gpu.py and tests/test_bf16_gpu.py as named rows (data only), each with the
kernel it declares for its forward and its backward pass: the names of mri3d_maxpool3d_route / mri3d_upsample3d_route
(include/mri3d.h).  tests/test_resample_routes.py checks, without a GPU, that every row reaches what it declares and which names no
row reaches.  Every case runs with batch size N; tensors are fresh allocations unless a row says otherwise."""
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
