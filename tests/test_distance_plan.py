"""CPU suite: the case table of the distance transform against the library's own launch plan (ops.edt_plan, host only), and a
sweep of the query showing that every corner of the plan has a row the GPU suite runs."""
import itertools

import pytest

import distance_cases as cases
from mri_epilepsy_diagnosis_amd import _lib, ops


@pytest.mark.parametrize("c", cases.EDT_CASES, ids=lambda c: c.name)
def test_row_gets_the_plan_it_states(c):
    plan = ops.edt_plan((c.n,) + c.shape)
    assert tuple(plan[k] for k in cases.PLAN_KEYS) == c.plan, plan
    assert plan["batch"] == c.n and plan["lds_bytes"] == (8192 + 2 * 256) * 4
    d, h, w = c.shape
    assert plan["ws_bytes"] == _lib.lib().mri3d_edt_workspace_bytes(c.n, d, h, w) >= 2 * 4 * c.n * d * h * w


def test_the_plan_is_what_the_header_says():
    # 2 x 160x192x160: 50 rows of 161 ints fit the tile of 8192; tiles of 32 lines of 192 and of 160 values
    p = ops.edt_plan((2, 160, 192, 160))
    assert (p["rows_w"], p["partial_w"], p["grid_w"]) == (50, 2 * 160 * 192 % 50, -(-2 * 160 * 192 // 50))
    assert (p["tx_h"], p["staged_h"], p["partial_h"], p["grid_h"]) == (32, 1, 0, 2 * 160 * 5)
    assert (p["tx_d"], p["staged_d"], p["partial_d"], p["grid_d"]) == (32, 1, 0, 2 * 192 * 160 // 32)
    # the tile narrows by powers of two as the line grows, and is given up past 8192 values
    assert [ops.edt_plan((1, h, 100))["tx_h"] for h in (256, 257, 512, 513, 4096, 4097, 8192, 8193)] == [32, 16, 16, 8, 2, 1, 1, 64]
    assert [ops.edt_plan((1, h, 100))["staged_h"] for h in (8192, 8193)] == [1, 0]
    assert [ops.edt_plan((1, 1, w))["staged_w"] for w in (8190, 8191, 8192)] == [1, 1, 0]
    # 2-D shapes are d = 1
    assert ops.edt_plan((37, 70)) == ops.edt_plan((1, 37, 70)) == ops.edt_plan((1, 1, 37, 70))


def test_no_corner_of_the_plan_lacks_a_row():
    covered = set()
    for c in cases.EDT_CASES:
        covered |= cases.plan_corners(ops.edt_plan((c.n,) + c.shape), c.n)
    extents = (1, 2, 3, 5, 31, 32, 33, 64, 65, 70, 160, 192, 257, 300, 4097, 8191, 8192, 8193, 20000)
    seen = set()
    for n, (d, h, w) in itertools.product((1, 3), itertools.product(extents, repeat=3)):
        if d * h * w >= 2 ** 31 or d * d + h * h + w * w >= ops.EDT_INF:
            continue
        seen |= cases.plan_corners(ops.edt_plan((n, d, h, w)), n)
    assert seen <= covered, sorted(seen - covered, key=str)
    assert len(seen) >= 14
