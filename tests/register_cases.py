"""Inputs and the case table shared by the registration tests (tests/test_register_*.py): Gaussian-smoothed noise volumes, affines
built from a rotation, per-axis scales and a shift about the grid centres, and one row per corner of the joint-histogram plan
(csrc/register.hip: 4 rows per block and trip, at most 512 blocks per candidate group, groups of 4 candidates, 64 voxels per wave
step)."""
import numpy as np
from scipy import ndimage


def smooth_noise(shape, seed, sigma=3.0):
    """Gaussian-smoothed white noise, scaled to unit standard deviation, float32."""
    rng = np.random.default_rng(seed)
    pad = [s + 4 * int(np.ceil(sigma)) for s in shape]
    v = ndimage.gaussian_filter(rng.standard_normal(pad), sigma, mode="wrap")
    v = v[tuple(slice(0, s) for s in shape)]
    return (v / v.std()).astype(np.float32)


def rotation(deg):
    rx, ry, rz = np.deg2rad(deg)
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def affine(fixed_shape, moving_shape, deg=(0, 0, 0), scales=(1, 1, 1), shift=(0, 0, 0)):
    """(3, 4) float32: fixed voxel -> moving voxel, rotation and scales about the fixed centre, centre to centre plus `shift`."""
    M = rotation(deg) @ np.diag(scales)
    cf, cm = (np.array(fixed_shape) - 1) / 2.0, (np.array(moving_shape) - 1) / 2.0
    return np.concatenate([M, (cm + np.array(shift) - M @ cf)[:, None]], 1).astype(np.float32)


def candidates(fixed_shape, moving_shape, k, seed, deg=(7, -5, 4), scales=(1.05, 0.97, 1.1), shift=(0, 0, 0)):
    """k affines: the named one, then small random perturbations of it (what a search step scores)."""
    rng = np.random.default_rng(seed)
    out = [affine(fixed_shape, moving_shape, deg, scales, shift)]
    for _ in range(k - 1):
        out.append(affine(fixed_shape, moving_shape, np.array(deg) + rng.uniform(-3, 3, 3), np.array(scales) * rng.uniform(0.97, 1.03, 3),
                          np.array(shift) + rng.uniform(-1.5, 1.5, 3)))
    return np.stack(out)


# name: (fixed shape, moving shape, k, bins, shift, fraction of fixed voxels masked out)
#   rows = d * h of the fixed grid; quads = ceil(rows / 4); blocks = min(quads, 512); trips = ceil(quads / blocks)
GENERAL_CASES = {
    "probe_k1_b32": ((40, 48, 36), (44, 40, 50), 1, 32, (0, 0, 0), 0.3),        # the issue's probe: 480 blocks, one candidate
    "k5_b16_w70": ((20, 24, 70), (24, 22, 75), 5, 16, (0, 0, 0), 0.3),          # groups of 4 + 1; w = 64 + 6
    "k64_b64": ((12, 14, 20), (14, 12, 22), 64, 64, (0, 0, 0), 0.2),            # 16 full groups, 64 KB of LDS
    "tiny_3_rows": ((1, 3, 5), (4, 4, 6), 2, 16, (0, 0, 0), 0.0),               # smaller than one block: wave 3 has no row
    "tail_45_rows": ((5, 9, 33), (6, 10, 30), 3, 32, (0, 0, 0), 0.2),           # 12 blocks, the last with one row
    "two_trips": ((48, 44, 8), (50, 40, 10), 1, 32, (0, 0, 0), 0.0),            # 528 quads on 512 blocks: blocks 0..15 go round twice
    "partial_overlap": ((24, 20, 30), (20, 24, 28), 4, 32, (6, -5, 9), 0.2),    # a part of every candidate's samples falls outside
    "no_mask_w128": ((6, 7, 128), (8, 8, 120), 1, 64, (0, 0, 0), 0.0),          # w a multiple of 64, nothing skipped
}


def plan_corners(fixed_shape, k, plan):
    """The corners of the launch plan a case sits on, from the plan's own fields (ops.JOINT_HIST_PLAN_FIELDS)."""
    rows = fixed_shape[0] * fixed_shape[1]
    corners = set()
    corners.add("one_trip" if plan["trips"] == 1 else "many_trips")
    corners.add("blocks_capped" if plan["blocks"] * plan["rows_per_trip"] < rows else "blocks_by_rows")
    corners.add("full_group" if plan["group_candidates"] == 4 else "short_group")
    corners.add("one_group" if plan["groups"] == 1 else "many_groups")
    if k > 4 and k % 4:
        corners.add("ragged_last_group")
    if rows % plan["rows_per_trip"]:
        corners.add("tail_rows")
    if rows < plan["rows_per_trip"]:
        corners.add("under_one_block")
    corners.add("w_whole_steps" if fixed_shape[2] % plan["wave_step"] == 0 else "w_tail_step")
    if fixed_shape[2] > plan["wave_step"]:
        corners.add("many_w_steps")
    return corners


ALL_CORNERS = {"one_trip", "many_trips", "blocks_capped", "blocks_by_rows", "full_group", "short_group", "one_group", "many_groups",
               "ragged_last_group", "tail_rows", "under_one_block", "w_whole_steps", "w_tail_step", "many_w_steps"}


def general_case(name):
    """(fixed_bins uint8, moving float32, affines (k, 3, 4) float32, m_lo, m_scale, bins) of a GENERAL_CASES row."""
    import register_ref
    fshape, mshape, k, bins, shift, masked = GENERAL_CASES[name]
    seed = sorted(GENERAL_CASES).index(name)
    fixed, moving = smooth_noise(fshape, 100 + seed), smooth_noise(mshape, 200 + seed)
    mask = None
    if masked:
        mask = smooth_noise(fshape, 300 + seed) > np.quantile(smooth_noise(fshape, 300 + seed), masked)
    f_lo, f_hi = np.percentile(fixed, [1, 99])
    m_lo, m_hi = np.percentile(moving, [1, 99])
    fixed_bins = register_ref.quantize(fixed, f_lo, bins / (f_hi - f_lo), bins, mask)
    return fixed_bins, moving, candidates(fshape, mshape, k, 400 + seed, shift=shift), float(np.float32(m_lo)), float(np.float32(bins / (m_hi - m_lo))), bins
