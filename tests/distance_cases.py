"""The cases of the distance-map suites (tests/test_distance_plan.py on the CPU, tests/test_distance_gpu.py on the device): the
shapes of the transform with the launch plan each must get, the mask patterns, and the inputs of the signed map and the loss."""
import collections
import functools

import numpy as np

EdtCase = collections.namedtuple("EdtCase", "name n shape patterns plan")
# plan: (rows_w, staged_w, partial_w, tx_h, staged_h, partial_h, tx_d, staged_d, partial_d, grid_w, grid_h, grid_d)
PLAN_KEYS = ("rows_w", "staged_w", "partial_w", "tx_h", "staged_h", "partial_h", "tx_d", "staged_d", "partial_d", "grid_w", "grid_h",
             "grid_d")

ALL = ("all_zero", "all_one", "corner_zero", "centre_zero", "one_voxel", "rand01", "rand50", "rand99", "ball", "half")
# a line too long for the tile is searched end to end wherever the search cannot stop early: only patterns with zeros near by
NEAR = ("all_zero", "rand50", "rand99")

EDT_CASES = [
    EdtCase("one_voxel_volume", 1, (1, 1, 1), ALL, (1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1)),
    EdtCase("one_row", 1, (1, 1, 70), ALL, (1, 1, 0, 32, 1, 6, 32, 1, 6, 1, 3, 3)),
    EdtCase("one_column_along_d", 1, (70, 1, 1), ALL, (70, 1, 0, 1, 1, 0, 1, 1, 0, 1, 70, 1)),
    EdtCase("a_2d_map", 1, (1, 37, 70), ALL, (37, 1, 0, 32, 1, 6, 32, 1, 30, 1, 3, 81)),
    EdtCase("long_rows", 1, (3, 5, 300), ALL, (15, 1, 0, 32, 1, 12, 32, 1, 28, 1, 30, 47)),
    EdtCase("long_along_d", 1, (300, 2, 3), ALL, (256, 1, 88, 4, 1, 3, 8, 1, 6, 3, 300, 1)),
    EdtCase("long_along_h", 1, (9, 257, 4), ALL, (256, 1, 9, 4, 1, 0, 32, 1, 4, 10, 9, 33)),
    EdtCase("odd_everywhere", 1, (17, 19, 23), ALL, (256, 1, 67, 32, 1, 23, 32, 1, 21, 2, 17, 14)),
    EdtCase("tile_multiples_and_one_over", 1, (33, 64, 65), ALL, (126, 1, 96, 32, 1, 1, 32, 1, 0, 17, 99, 130)),
    EdtCase("batch_of_three", 3, (6, 9, 40), ALL, (162, 1, 0, 32, 1, 8, 32, 1, 8, 1, 36, 36)),
    EdtCase("w_too_long_to_stage", 1, (1, 2, 8200), ALL, (1, 0, 0, 32, 1, 8, 32, 1, 16, 2, 257, 513)),
    EdtCase("h_too_long_to_stage", 1, (2, 8200, 3), ALL, (256, 1, 16, 64, 0, 3, 32, 1, 24, 65, 2, 769)),
    EdtCase("h_too_long_whole_tile", 1, (1, 8200, 64), NEAR, (126, 1, 10, 64, 0, 0, 32, 1, 0, 66, 1, 16400)),
    EdtCase("d_too_long_to_stage", 1, (8200, 1, 2), ALL, (256, 1, 8, 2, 1, 0, 64, 0, 2, 33, 8200, 1)),
    EdtCase("d_too_long_whole_tile", 1, (8200, 1, 64), NEAR, (126, 1, 10, 32, 1, 0, 64, 0, 0, 66, 16400, 1)),
]


def plan_corners(plan, n):
    """The corners of a plan: per pass whether its lines are staged, whether the last tile is partial, and whether the tile is
    narrower than the widest; and whether there is more than one volume."""
    return {("w", plan["staged_w"], plan["partial_w"] > 0),
            ("h", plan["staged_h"], plan["partial_h"] > 0, plan["tx_h"] < 32),
            ("d", plan["staged_d"], plan["partial_d"] > 0, plan["tx_d"] < 32),
            ("batch", n > 1)}


def pattern(name, shape, seed=0):
    """A uint8 (d, h, w) mask."""
    d, h, w = shape
    rng = np.random.default_rng(seed)
    m = np.ones(shape, np.uint8)
    if name == "all_zero":
        m[:] = 0
    elif name == "all_one":
        pass
    elif name == "corner_zero":
        m[0, 0, 0] = 0
    elif name == "centre_zero":
        m[d // 2, h // 2, w // 2] = 0
    elif name == "one_voxel":
        m[:] = 0
        m[d - 1 - d // 3, h // 3, w - 1 - w // 4] = 3
    elif name.startswith("rand"):
        m = (rng.random(shape) < int(name[4:]) / 100.0).astype(np.uint8) * 255
    elif name == "ball":
        g = np.ogrid[:d, :h, :w]
        r = max(1.0, 0.4 * min(s for s in shape if s > 1)) if max(shape) > 1 else 1.0
        m = (sum((a - (s - 1) / 2.0) ** 2 for a, s in zip(g, shape)) <= r * r).astype(np.uint8)
    elif name == "half":
        axis = int(np.argmax(shape))
        idx = [slice(None)] * 3
        idx[axis] = slice(shape[axis] // 2, None)
        m[tuple(idx)] = 0
    else:
        raise KeyError(name)
    return m


def hole_masks():
    """name -> mask for fill_holes: a closed shell, a ring in a 2-D map, and a cavity that reaches the border."""
    shell = np.zeros((9, 10, 11), np.uint8)
    shell[2:7, 2:8, 2:9] = 1
    shell[3:6, 3:7, 3:8] = 0
    ring = np.zeros((12, 15), np.uint8)
    ring[2:10, 3:12] = 1
    ring[4:8, 5:10] = 0
    ring[5, 6] = 1                                   # an island in the hole
    open_cavity = shell.copy()
    open_cavity[4, 4, :5] = 0                        # a tunnel from the cavity to the w = 0 face
    two = np.zeros((8, 20, 20), np.uint8)
    two[1:7, 1:9, 1:9] = 1
    two[2:6, 2:8, 2:8] = 0
    two[1:7, 11:19, 11:19] = 1
    two[3:5, 13:17, 13:17] = 0
    return {"shell": shell, "ring_2d": ring, "open_cavity": open_cavity, "two_shells": two}


LOSS_CLASSES = [(2, (1,)), (3, (0, 1)), (9, (1, 2, 5)), (32, tuple(range(32)))]
LOSS_SPATIAL = [(5, 6, 7), (8, 16, 33), (1, 20, 70)]


def class_map(C, spatial, seed, n=2, block=3):
    """uint8 (n, d, h, w): classes in blocks of `block` voxels, so distances reach a few voxels."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, C, (n,) + tuple(-(-s // block) for s in spatial)).astype(np.uint8)
    y = np.kron(coarse, np.ones((1, block, block, block), np.uint8))
    return np.ascontiguousarray(y[:, :spatial[0], :spatial[1], :spatial[2]])


@functools.lru_cache(maxsize=None)
def _loss_inputs(C, spatial, scale, seed, n):
    rng = np.random.default_rng(1000 + seed)
    z = rng.standard_normal((n, C) + tuple(spatial)) * scale
    return z, class_map(C, spatial, seed, n)


def loss_inputs(C, spatial, scale, seed=0, n=2):
    """(float64 logits (n, C, d, h, w), uint8 class map (n, d, h, w)), fresh copies."""
    z, y = _loss_inputs(C, tuple(spatial), float(scale), seed, n)
    return z.copy(), y.copy()


def signed_map_cases():
    """name -> (class map (n, d, h, w), C): what the signed map must get right beyond plain blobs."""
    out = {}
    y = class_map(3, (7, 9, 10), 5)
    y[1][y[1] == 1] = 2
    out["absent_from_one_volume"] = (y, 3)
    y = class_map(3, (7, 9, 10), 6)
    y[0] = 1
    out["filling_a_volume"] = (y, 3)
    y = class_map(9, (7, 9, 10), 7)
    rng = np.random.default_rng(8)
    y[rng.random(y.shape) < 0.1] = 255
    out["ignored_scattered"] = (y, 9)
    out["all_ignored"] = (np.full((2, 4, 5, 6), 255, np.uint8), 2)
    y = np.full((2, 4, 5, 6), 1, np.uint8)
    y[0, 1, 2, 3] = 255
    y[1, 0, 0, 0] = 0
    out["filling_all_counted_voxels"] = (y, 2)
    return out
