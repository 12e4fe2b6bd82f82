"""CPU suite: tests/register_ref.py, the float64 / float32 restatement of csrc/register.hip, held to independent code (scikit-learn,
scipy.ndimage, plain reshapes), and its certain / uncertain containment held to the float32 emulation of the kernel and to six
planted mistakes that must fall outside it."""
import numpy as np
import pytest
from scipy import ndimage
from sklearn.metrics import mutual_info_score

import register_cases as RC
import register_ref as R


@pytest.fixture(scope="module")
def probe():
    return RC.general_case("probe_k1_b32")


def _contained(H, bounds, c=0):
    Hc, Hp, nc, nu = bounds
    return bool((Hc[c] <= H).all() and (H <= Hc[c] + Hp[c]).all() and nc[c] <= H.sum() <= nc[c] + nu[c])


def test_mutual_information_matches_sklearn(probe):
    fb, moving, A, m_lo, m_scale, bins = probe
    H = R.joint_hist(fb, moving, A, m_lo, m_scale, bins)
    got = R.hist_costs(H, 1)
    assert got[0, 1] == H[0].sum() > 1000
    assert got[0, 0] == pytest.approx(-mutual_info_score(None, None, contingency=H[0]), rel=1e-10)
    p = H[0] / H[0].sum()
    ent = lambda q: -(q[q > 0] * np.log(q[q > 0])).sum()   # noqa: E731
    assert R.hist_costs(H, 2)[0, 0] == pytest.approx(-(ent(p.sum(1)) + ent(p.sum(0))) / ent(p.ravel()), rel=1e-12)


def test_correlation_ratio_of_known_tables():
    H = np.zeros((1, 4, 4), dtype=np.int64)
    H[0, 0, 1] = H[0, 1, 3] = H[0, 2, 0] = 5                  # y is a function of the fixed bin: nothing left to explain
    assert abs(R.hist_costs(H, 0)[0, 0]) < 1e-28
    H[0] = 3                                                   # independent: every row has the whole variance
    assert R.hist_costs(H, 0)[0, 0] == pytest.approx(1.0, rel=1e-14)
    H[0] = 0
    H[0, :, 2] = 7                                             # one moving bin: no variance to explain
    assert np.isinf(R.hist_costs(H, 0)[0, 0]) and R.hist_costs(H, 1)[0, 0] == pytest.approx(0.0, abs=1e-15)
    H[0] = 0
    H[0, 1, 1] = 9                                             # one cell: H_fm = 0
    assert np.isinf(R.hist_costs(H, 2)[0, 0])
    assert np.isinf(R.hist_costs(H, 1, min_count=10)[0, 0]) and R.hist_costs(H, 1, min_count=9)[0, 0] == 0.0
    assert np.isinf(R.hist_costs(np.zeros((1, 4, 4), dtype=np.int64), 1)[0, 0])


def test_resampling_matches_scipy_in_the_interior():
    img = RC.smooth_noise((14, 16, 12), 1)
    lab = (np.random.default_rng(2).integers(0, 200, (14, 16, 12))).astype(np.uint8)
    A = RC.affine((11, 13, 15), img.shape, deg=(6, -4, 9), scales=(1.1, 0.9, 0.8), shift=(0.3, -0.7, 0.2))
    out_i, out_l = R.resample_affine(img, lab, A, (11, 13, 15), pad=-3.0)
    A64 = A.astype(np.float64)
    ref_i = ndimage.affine_transform(img.astype(np.float64), A64[:, :3], A64[:, 3], (11, 13, 15), order=1, mode="nearest")
    ref_l = ndimage.affine_transform(lab, A64[:, :3], A64[:, 3], (11, 13, 15), order=0, mode="nearest")
    s = R.coords(A, (11, 13, 15))
    interior = np.ones((11, 13, 15), dtype=bool)
    for a in range(3):
        interior &= (s[a] >= 0) & (s[a] <= img.shape[a] - 1)
    sure_in, sure_out, dv, tie = R.resample_bounds(img, A, (11, 13, 15))
    assert interior.sum() > 500 and (sure_in | sure_out).all()
    np.testing.assert_allclose(out_i[interior], ref_i[interior], rtol=0, atol=1e-12)
    assert (out_l[interior & ~tie] == ref_l[interior & ~tie]).all() and tie.mean() < 0.01
    assert (out_i[sure_out] == -3.0).all() and (out_l[sure_out] == 0).all() and sure_out.any()


def test_pyramid_is_a_reshape_mean_on_even_shapes_and_counts_what_exists():
    x = RC.smooth_noise((8, 10, 6), 3)
    ref = x.astype(np.float64).reshape(4, 2, 5, 2, 3, 2).mean((1, 3, 5))
    np.testing.assert_allclose(R.downsample2(x), ref, rtol=1e-15)
    assert np.abs(R.downsample2(x, fp32=True) - ref).max() <= 8 * 2.0 ** -24 * np.abs(x).max()
    odd = np.arange(3 * 5 * 1, dtype=np.float32).reshape(3, 5, 1)
    y = R.downsample2(odd)
    assert y.shape == (2, 3, 1) and y[0, 0, 0] == odd[:2, :2].mean() and y[1, 2, 0] == odd[2, 4, 0] and y[0, 2, 0] == odd[:2, 4].mean()


def test_identity_on_equal_grids_gives_a_diagonal_histogram():
    v = RC.smooth_noise((9, 10, 11), 4)
    lo, hi = np.percentile(v, [1, 99])
    lo32, sc32 = np.float32(lo), np.float32(16 / (hi - lo))
    fb = R.quantize(v, lo32, sc32, 16)
    eye = RC.affine(v.shape, v.shape)
    for fp32 in (False, True):
        H = R.joint_hist(fb, v, eye, lo32, sc32, 16, fp32=fp32)[0]
        assert H.sum() == v.size and (H == np.diag(np.bincount(fb.ravel(), minlength=16))).all()
    fb[2] = R.SKIP
    assert R.joint_hist(fb, v, eye, lo32, sc32, 16)[0].sum() == v.size - 10 * 11


def test_quantize_skips_masked_and_non_finite_voxels():
    x = np.array([-5.0, 0.0, 0.49, 0.5, 7.9, 8.0, 100.0, np.nan, np.inf, 3.0], dtype=np.float32)
    mask = np.ones(10, dtype=np.uint8)
    mask[9] = 0
    assert R.quantize(x, 0.0, 2.0, 16, mask).tolist() == [0, 0, 0, 1, 15, 15, 15, 255, 255, 255]


def test_fp32_emulation_stays_inside_the_containment_and_few_samples_are_uncertain(probe):
    fb, moving, A, m_lo, m_scale, bins = probe
    bounds = R.joint_hist_bounds(fb, moving, A, m_lo, m_scale, bins)
    assert bounds[3][0] <= 0.01 * bounds[2][0] and bounds[2][0] > 10000
    assert _contained(R.joint_hist(fb, moving, A, m_lo, m_scale, bins, fp32=True)[0], bounds)
    assert _contained(R.joint_hist(fb, moving, A, m_lo, m_scale, bins, fp32=False)[0], bounds)


MISTAKES = ["transposed_affine", "half_voxel_shift", "swapped_axes", "strict_inside_rule", "skip_counted", "bins_off_by_one"]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_planted_mistakes_fall_outside_the_containment(probe, mistake):
    fb, moving, A, m_lo, m_scale, bins = probe
    bounds = R.joint_hist_bounds(fb, moving, A, m_lo, m_scale, bins)
    A2, fb2, kw = A.copy(), fb, {}
    if mistake == "transposed_affine":
        A2[0, :, :3] = A[0, :, :3].T
    elif mistake == "half_voxel_shift":
        A2[0, :, 3] += 0.5
    elif mistake == "strict_inside_rule":
        kw = dict(inside_lo=0.0, inside_hi=-1.0)                 # 0 <= s <= N - 1: the half-voxel border is lost
    elif mistake == "skip_counted":
        fb2 = np.where(fb == R.SKIP, 0, fb).astype(np.uint8)
    H = R.joint_hist(fb2, moving, A2, m_lo, m_scale, bins, fp32=True, **kw)[0]
    if mistake == "swapped_axes":
        H = H.T.copy()
    elif mistake == "bins_off_by_one":
        H = np.roll(H, 1, axis=1)
    assert not _contained(H, bounds)
