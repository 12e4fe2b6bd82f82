"""References of the intensity statistics (csrc/intensity.hip, classification/intensity.py, preprocessing.train_landmarks), all numpy
float64 on the CPU.

kde_ref is scipy.stats.gaussian_kde's closed form for one-dimensional data,
    density[j] = sum_i exp(-(p_j - x_i)^2 / 2h^2) / (n sqrt(2 pi h^2)),   h^2 = var(x, ddof=1) * factor^2,
    factor = n^(-1/5) (Scott), (3n/4)^(-1/5) (Silverman) or a given number,
over the voxels a mask selects.  Its float32 mode rounds where the kernel rounds: the centred, scaled voxels and positions
(x - mean) sqrt(log2 e / 2h^2) are rounded to float32, difference, square and exp2 are float32 operations, and the terms of each run
of RUN = 256 consecutive voxels of the row (masked-out ones adding an exact 0) are added one after the other in float32; the run
sums are added in float64.  `fault` plants one of four mistakes a kernel of this kind can make, for tests/test_intensity.py to show
that the GPU bound would see them.
"""
import numpy as np

RUN = 256          # voxels whose terms the kernel adds in float32 before the sum goes to float64 (intensity.hip: kKdeRun)
TILE = 1024        # voxels per tile (kKdeTile)
MAX_BLOCKS = 1024  # blocks per row (kIntMaxBlocks)
FAULTS = ("biased_variance", "silverman_for_scott", "dropped_tail_tile", "step_over_m")
STANDARD_RANGE = 0, 100
DEFAULT_CUTOFF = 0.01, 0.99


def t1_like(seed, shape):
    """Skull-stripped-T1-like float32 intensities: 45 % exact zeros, grey- and white-matter modes."""
    rng = np.random.default_rng(seed)
    grey, white = rng.normal(450.0, 60.0, size=shape), rng.normal(700.0, 45.0, size=shape)
    tissue = np.abs(np.where(rng.random(shape) < 0.55, grey, white))
    return np.where(rng.random(shape) < 0.45, 0.0, tissue).astype(np.float32)


def kde_plan(n, m):
    """(blocks per row, voxels per tile, position slots per lane, trips of a block's tile loop): what mri3d_kde_plan must report."""
    tiles = -(-n // TILE)
    blocks = min(tiles, MAX_BLOCKS)
    slots = 1
    while slots * 64 < m:
        slots *= 2
    return blocks, TILE, slots, -(-tiles // blocks)


def moments_ref(x, mask=None):
    """[count, non-finite count, min, max, mean, unbiased variance, 0, 0] of the voxels `mask` selects, the last four over the
    finite ones; mean and variance in two passes, as np.cov takes them."""
    v = np.asarray(x).reshape(-1)
    if mask is not None:
        v = v[np.asarray(mask).reshape(-1).astype(bool)]
    v = v.astype(np.float64)
    fin = v[np.isfinite(v)]
    out = np.zeros(8)
    out[0], out[1] = v.size, v.size - fin.size
    out[2] = fin.min() if fin.size else np.inf
    out[3] = fin.max() if fin.size else -np.inf
    out[4] = fin.sum() / fin.size if fin.size else np.nan
    out[5] = ((fin - out[4]) ** 2).sum() / (fin.size - 1) if fin.size >= 2 else np.nan
    return out


def factor_ref(count, bw_method):
    if bw_method is None or bw_method == "scott":
        return np.power(float(count), -1.0 / 5.0)
    if bw_method == "silverman":
        return np.power(count * 3.0 / 4.0, -1.0 / 5.0)
    return float(bw_method)


def kde_ref(x, num_positions=100, positions=None, bw_method=None, mask=None, float32=False, fault=None):
    """(positions, density) float64 of one volume; NaN densities where scipy has no answer."""
    assert fault is None or fault in FAULTS
    row = np.asarray(x).reshape(-1)
    keep = np.ones(row.size, bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    mom = moments_ref(row, keep)
    count, bad, lo, hi, mean, var = mom[:6]
    m = num_positions if positions is None else len(positions)
    if positions is None:
        with np.errstate(all="ignore"):
            positions = lo + np.arange(m) * ((hi - lo) / m) if fault == "step_over_m" else np.linspace(lo, hi, num=m)
    positions = np.asarray(positions, dtype=np.float64)
    if count < 2 or bad > 0 or not var > 0:
        return positions, np.full(m, np.nan)
    if fault == "biased_variance":
        var = var * (count - 1) / count
    factor = factor_ref(count, "silverman" if fault == "silverman_for_scott" and bw_method in (None, "scott") else bw_method)
    h2 = var * factor * factor
    if fault == "dropped_tail_tile" and row.size % TILE:
        keep = keep.copy()
        keep[row.size // TILE * TILE:] = False
    total = np.zeros(m)
    if not float32:
        v = row[keep].astype(np.float64)
        step = max(1, 4_000_000 // m)
        for i in range(0, v.size, step):
            d = positions[None, :] - v[i:i + step, None]
            total += np.exp(-(d * d) / (2.0 * h2)).sum(axis=0)
    else:
        scale = np.sqrt(np.log2(np.e) / (2.0 * h2))
        xs = ((row.astype(np.float64) - mean) * scale).astype(np.float32)
        xs[~keep] = np.inf                                           # exp2(-inf) = 0
        ps = ((positions - mean) * scale).astype(np.float32)
        runs = -(-xs.size // RUN)
        xs = np.concatenate([xs, np.full(runs * RUN - xs.size, np.inf, np.float32)]).reshape(runs, RUN)
        step = max(1, 4_000_000 // (RUN * m))
        for i in range(0, runs, step):
            d = ps[None, None, :] - xs[i:i + step, :, None]
            terms = np.exp2(-(d * d))
            assert terms.dtype == np.float32
            total += np.cumsum(terms, axis=1, dtype=np.float32)[:, -1, :].astype(np.float64).sum(axis=0)
    return positions, total / (count * np.sqrt(2.0 * np.pi * h2))


# ------------------------------------------------------------------------------------------------ the cases of the two suites
# name: (voxels, data, masked, m, bw_method).  data: 't1' = t1_like, 'scanner' = the same x 20 + 17.3 (a raw-scanner range),
# 'offset' = the same + 1e4 (the variance is a small difference of large sums), 'pair' = two voxels.  masked: x > mean(x).
# What each size exercises is in the docstring of tests/test_intensity_gpu.py; n * m stays below 6e7.
CASES = {
    "two_voxels": (2, "pair", False, 100, None),
    "one_tile_masked": (5 * 7 * 9, "t1", True, 100, None),
    "blocks_t1": (7 * 11 * 37, "t1", False, 100, None),
    "blocks_scanner_silverman": (7 * 11 * 37, "scanner", False, 100, "silverman"),
    "blocks_offset_factor": (7 * 11 * 37, "offset", False, 100, 0.3),
    "blocks_scanner_masked": (7 * 11 * 37, "scanner", True, 65, None),
    "many_blocks_offset": (81 ** 3, "offset", False, 64, None),
    "second_trip_masked": (1024 * 1024 + 315, "scanner", True, 28, "silverman"),
    "third_trip": (129 ** 3, "t1", False, 3, None),
}
CASES.update({"slots_m%d" % m: (5 * 7 * 9, "t1", False, m, None) for m in (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024)})
SMALL_CASES = [k for k, v in CASES.items() if v[0] * v[3] <= 400_000]
_cache = {}


def case_data(name):
    """(x, mask): the float32 row of the case and its boolean mask (None without one)."""
    n, data, masked, _, _ = CASES[name]
    if data == "pair":
        x = np.array([450.25, 700.5], np.float32)
    else:
        x = t1_like(1000 + n % 997, (n,))
        if data == "scanner":
            x = (x * np.float32(20.0) + np.float32(17.3)).astype(np.float32)
        elif data == "offset":
            x = (x + np.float32(1.0e4)).astype(np.float32)
    return x, (x > x.mean()) if masked else None


def case_refs(name):
    """The float64 reference of a case, computed once: positions, density, the error e32 of the float32 mode and the bound of the
    GPU suite, 8 max(e32, 2^-23 max(density))."""
    if name not in _cache:
        _, _, _, m, bw = CASES[name]
        x, mask = case_data(name)
        pos, d64 = kde_ref(x, m, bw_method=bw, mask=mask)
        _, d32 = kde_ref(x, m, bw_method=bw, mask=mask, float32=True)
        e32 = float(np.abs(d32 - d64).max())
        _cache[name] = {"positions": pos, "density": d64, "e32": e32, "bound": 8.0 * max(e32, 2.0 ** -23 * float(d64.max())),
                        "moments": moments_ref(x, mask)}
    return _cache[name]


def average_mapping_ref(percentiles_database):
    """The landmark vector of a (images, percentiles) database: each image's first / last percentile go to 0 / 100 by a line of its
    own; the landmarks are the mean over images of the lines at their percentiles, as one dot product."""
    db = np.asarray(percentiles_database, dtype=np.float64)
    s1, s2 = STANDARD_RANGE
    slopes = np.nan_to_num((s2 - s1) / (db[:, -1] - db[:, 0]))
    intercepts = np.mean(s1 - slopes * db[:, 0])
    return slopes.dot(db) / len(db) + intercepts


def percentiles_ref(cutoff=None):
    lo, hi = DEFAULT_CUTOFF if cutoff is None else cutoff
    lo, hi = min(max(0.0, lo), 0.09), max(min(1.0, hi), 0.91)
    cut = 100 * np.array([lo, hi])
    return np.array(sorted(set(list(cut) + list(range(25, 100, 25)) + list(range(10, 100, 10)))))


def train_landmarks_ref(arrays, cutoff=None, masks=None):
    """Landmarks of float32 arrays: np.percentile of each array's selected voxels at the 13 percentiles, then the average mapping."""
    masks = [None] * len(arrays) if masks is None else masks
    pct = percentiles_ref(cutoff)
    rows = []
    for a, k in zip(arrays, masks):
        v = np.asarray(a, dtype=np.float32).reshape(-1)
        rows.append(np.percentile(v if k is None else v[np.asarray(k).reshape(-1).astype(bool)], pct))
    return average_mapping_ref(np.vstack(rows))
