"""The case table of the connected-components tests, built from the plan query (ops.components_plan), not from constants: with
T = (td, th, tw) the tile the query reports, the volumes sit below, at and above a tile per axis, put voxel pairs across tile faces,
edges and corners, and thread one component through every tile.  Every volume stays far below a million voxels.

A case is (name, uint8 mask, by_value, expect) with expect None or {connectivity: K}, a count known without the reference."""
import collections

import numpy as np

from mri_epilepsy_diagnosis_amd import ops

Case = collections.namedtuple("Case", "name mask by_value expect")


def tile():
    p = ops.components_plan((1, 1, 1), 6)
    return p["td"], p["th"], p["tw"]


def _bernoulli(rng, shape, p):
    return (rng.random(shape) < p).astype(np.uint8)


def _pair(shape, a, b):
    m = np.zeros(shape, dtype=np.uint8)
    m[a] = m[b] = 1
    return m


def _snake(shape):
    """A one-voxel-wide boustrophedon path: full rows at even (z, y), joined at alternating ends, the planes joined at alternating
    ends of the in-plane path.  Rows and planes between carry the connectors only."""
    d, h, w = shape
    m = np.zeros(shape, dtype=np.uint8)
    plane = np.zeros((h, w), dtype=np.uint8)
    rows = list(range(0, h, 2))
    for j, y in enumerate(rows):
        plane[y, :] = 1
        if j + 1 < len(rows):
            plane[y + 1, w - 1 if j % 2 == 0 else 0] = 1
    end = (rows[-1], w - 1 if (len(rows) - 1) % 2 == 0 else 0)     # the path starts at (0, 0) and ends here
    planes = list(range(0, d, 2))
    for k, z in enumerate(planes):
        m[z] = plane
        if k + 1 < len(planes):
            m[(z + 1,) + (end if k % 2 == 0 else (0, 0))] = 1
    return m


def _combs(shape):
    """Two interleaved combs: teeth are the planes x = 0 mod 4 (comb A, rows 0 .. h-3) and x = 2 mod 4 (comb B, rows 2 .. h-1); each
    comb's teeth meet only in its backbone, a row of the LAST plane z = d-1 (row 0 for A, row h-1 for B).  Two components."""
    d, h, w = shape
    m = np.zeros(shape, dtype=np.uint8)
    m[:, :h - 2, 0::4] = 1
    m[:, 2:, 2::4] = 1
    m[d - 1, 0, :] = 1
    m[d - 1, h - 1, :] = 1
    return m


def build():
    td, th, tw = T = tile()
    rng = np.random.default_rng(20240)
    cases = []

    def add(name, mask, by_value=False, expect=None):
        cases.append(Case(name, np.ascontiguousarray(mask, dtype=np.uint8), by_value, expect))

    near = (td + 1, th + 1, tw + 1)
    add("zeros", np.zeros(near), expect={6: 0, 18: 0, 26: 0})
    add("ones", np.ones(near), expect={6: 1, 18: 1, 26: 1})
    corners = np.zeros((td + 2, th + 2, tw + 2))
    corners[::td + 1, ::th + 1, ::tw + 1] = 1
    add("corners", corners, expect={6: 8, 18: 8, 26: 8})
    for shape in ((3, 5, 7), (1, 1, 1), (1, 9, 70), (5, 1, 1)):
        add("small_%dx%dx%d" % shape, np.ones(shape) if shape == (1, 1, 1) else _bernoulli(rng, shape, 0.5))
    add("map_2d_9x70", _bernoulli(rng, (9, 70), 0.5))                       # a 2-D map: d = 1 by shape
    add("one_tile", _bernoulli(rng, T, 0.45))
    for axis in range(3):
        shape = tuple(T[i] + (i == axis) for i in range(3))
        add("tile_plus_one_axis%d" % axis, _bernoulli(rng, shape, 0.45))
    add("two_tiles_plus_one", _bernoulli(rng, (2 * td + 1, 2 * th + 1, 2 * tw + 1), 0.45))

    # two voxels that touch only across a tile boundary; a = the voxel before the boundary on the crossed axes
    two = (2 * td, 2 * th, 2 * tw)
    mid = (td // 2, th // 2, tw // 2)
    for axis in range(3):                                                   # by a face
        a = tuple(T[i] - 1 if i == axis else mid[i] for i in range(3))
        b = tuple(T[i] if i == axis else mid[i] for i in range(3))
        add("face_axis%d" % axis, _pair(two, a, b), expect={6: 1, 18: 1, 26: 1})
    for free in range(3):                                                   # by an edge: both diagonals of the axis pair
        p, q = [i for i in range(3) if i != free]
        for flip in (0, 1):
            a, b = list(mid), list(mid)
            a[p], b[p] = T[p] - 1, T[p]
            a[q], b[q] = (T[q] - 1, T[q]) if not flip else (T[q], T[q] - 1)
            add("edge_axes%d%d_%s" % (p, q, "anti" if flip else "diag"), _pair(two, tuple(a), tuple(b)), expect={6: 2, 18: 1, 26: 1})
    for fy in (0, 1):                                                       # by a corner: the four space diagonals
        for fx in (0, 1):
            a = (td - 1, th if fy else th - 1, tw if fx else tw - 1)
            b = (td, th - 1 if fy else th, tw - 1 if fx else tw)
            add("corner_%d%d" % (fy, fx), _pair(two, a, b), expect={6: 2, 18: 2, 26: 1})

    z, y, x = np.indices(near)
    board = ((z + y + x) % 2 == 0)
    add("checkerboard", board, expect={6: int(board.sum()), 18: 1, 26: 1})
    assert board.sum() == (board.size + 1) // 2
    three = (3 * td, 3 * th, 3 * tw)
    add("snake", _snake(three), expect={6: 1, 18: 1, 26: 1})
    add("snake_complement", 1 - _snake(three))
    add("combs", _combs((2 * td + 1, th + 3, 2 * tw + 1)), expect={6: 2, 18: 2, 26: 2})
    for p in (0.3, 0.6):
        add("bernoulli_%.1f_tiles" % p, _bernoulli(rng, (2 * td + 3, 2 * th + 1, 3 * tw + 5), p))
        add("bernoulli_%.1f_24x40x72" % p, _bernoulli(rng, (24, 40, 72), p))
    blocks = rng.choice(np.array([0, 1, 2, 7, 255], dtype=np.uint8), size=(6, 7, 14))
    class_map = np.kron(blocks, np.ones((3, 3, 5), dtype=np.uint8))[:2 * td + 1, :2 * th + 3, :2 * tw + 5]
    add("class_map_by_value", class_map, by_value=True)
    add("class_map_as_mask", class_map)
    add("values_by_value", _bernoulli(rng, (td + 3, 2 * th + 1, tw + 9), 0.7) * rng.integers(1, 4, (td + 3, 2 * th + 1, tw + 9)), by_value=True)
    add("values_above_one", _bernoulli(rng, (td + 3, th + 1, 2 * tw + 1), 0.4) * rng.integers(1, 256, (td + 3, th + 1, 2 * tw + 1)))
    return cases


CONNECTIVITIES = (6, 18, 26)
