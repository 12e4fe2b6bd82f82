"""CPU suite of the intensity statistics (csrc/intensity.hip, ops.intensity_moments / gaussian_kde, classification/intensity.py,
preprocessing.train_landmarks): the references the GPU suite compares with are themselves checked (tests/intensity_ref.py against
scipy, against the records of tests/golden/intensity_stats.npz that tools/gen_intensity_golden.py made from the reference's own
`_get_average_mapping` and from scipy), the bound of the GPU suite is shown to see four planted mistakes, and the C ABI is
exercised where it needs no device (host-only queries, every validation branch, all before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import intensity_ref
from mri_epilepsy_diagnosis_amd import _lib, ops
from mri_epilepsy_diagnosis_amd.classification import intensity, preprocessing
from mri_epilepsy_diagnosis_amd.segmentation import transforms
from oracle import preprocessing as oracle_preprocessing
from util import load_golden

EINVAL, EWORKSPACE = -1, -4
P = ctypes.c_void_p
A, B, C_, D, E, F = 0x10000, 0x2000000, 0x4000000, 0x6000000, 0x8000000, 0xA000000     # non-NULL, far apart: never dereferenced
BANDWIDTHS = {"scott": None, "silverman": "silverman", "f03": 0.3}
REL_TO_MAX = 1e-10          # restatement against scipy; the two agree to 1e-12 at n = 200 000


def _rel_to_max(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("bw", list(BANDWIDTHS))
def test_restatement_is_scipy(bw, masked):
    stats = pytest.importorskip("scipy.stats")
    x = intensity_ref.t1_like(7, (11, 13, 14)) * np.float32(3.0) + np.float32(5.5)
    mask = (x > x.mean()) if masked else None
    values = x[mask] if masked else x.ravel()
    positions = np.linspace(np.float64(values.min()), np.float64(values.max()), num=100)      # float64 positions, see DESIGN 4.12
    want = stats.gaussian_kde(values, bw_method=BANDWIDTHS[bw])(positions)
    pos, got = intensity_ref.kde_ref(x, 100, bw_method=BANDWIDTHS[bw], mask=mask)
    assert np.array_equal(pos, positions)
    assert _rel_to_max(got, want) <= REL_TO_MAX
    _, given = intensity_ref.kde_ref(x, positions=positions[::7], bw_method=BANDWIDTHS[bw], mask=mask)
    assert _rel_to_max(given, want[::7]) <= REL_TO_MAX


@pytest.mark.parametrize("tag", ["all", "mask"])
@pytest.mark.parametrize("vol", ["a", "b", "c"])
def test_restatement_is_the_recorded_scipy(vol, tag):
    gold = load_golden("intensity_stats.npz")
    x = gold["vol_" + vol]
    mask = (x > x.ravel().mean()) if tag == "mask" else None
    for bw, method in BANDWIDTHS.items():
        pos, got = intensity_ref.kde_ref(x, 100, bw_method=method, mask=mask)
        assert np.array_equal(pos, gold["pos_%s_%s" % (vol, tag)])                      # np.linspace, bit for bit
        assert _rel_to_max(got, gold["kde_%s_%s_%s" % (vol, tag, bw)]) <= REL_TO_MAX, (vol, tag, bw)


def test_moments_reference_is_numpy():
    x = intensity_ref.t1_like(3, (4000,)) + np.float32(1.0e4)
    mask = x > x.mean()
    mom = intensity_ref.moments_ref(x, mask)
    v = x[mask].astype(np.float64)
    assert mom[0] == v.size and mom[1] == 0 and mom[2] == v.min() and mom[3] == v.max()
    assert abs(mom[4] - v.mean()) <= 1e-12 * abs(v.mean()) and abs(mom[5] - np.cov(v)) <= 1e-12 * np.cov(v)
    x[5] = np.nan
    x[6] = np.inf
    mom = intensity_ref.moments_ref(x)
    assert mom[0] == 4000 and mom[1] == 2 and np.isfinite(mom[2:6]).all()
    assert np.isnan(intensity_ref.moments_ref(x[:1])[5]) and intensity_ref.moments_ref(np.zeros(9, np.float32))[5] == 0


def test_average_mapping_is_the_reference_record_bit_for_bit():
    gold = load_golden("intensity_stats.npz")
    for db, want in ((gold["database"], gold["mapping"]), (gold["database_flat"], gold["mapping_flat"])):
        with np.errstate(all="ignore"):
            assert np.array_equal(intensity_ref.average_mapping_ref(db), want, equal_nan=True)
            assert np.array_equal(preprocessing._get_average_mapping(db), want, equal_nan=True)
    assert gold["mapping"].shape == (13,) and abs(gold["mapping"][0]) < 1e-9 and abs(gold["mapping"][-1] - 100) < 1e-9


def test_percentiles_of_the_reference_are_those_of_the_product():
    for cutoff in (None, (0.01, 0.99), (0.0, 1.0), (0.2, 0.8), (-1.0, 2.0)):
        cut = preprocessing.DEFAULT_CUTOFF if cutoff is None else cutoff
        want = preprocessing._get_percentiles(100 * np.array(preprocessing._standardize_cutoff(cut)))
        assert np.array_equal(intensity_ref.percentiles_ref(cutoff), want)


def test_landmarks_of_one_volume_map_its_cutoffs_to_the_standard_range():
    """Trained on one volume, the landmarks are that volume's own line: `normalize` (its float64 restatement, oracle/preprocessing.py)
    then sends the volume's 1st / 99th percentile to 0 / 100.  The output is stored as float32: half an ulp of 100 is 3.8e-6, and the
    percentile of the output interpolates between two such values; 1e-4 leaves room for both."""
    x = intensity_ref.t1_like(11, (12, 14, 16))
    landmarks = intensity_ref.train_landmarks_ref([x])
    assert landmarks.shape == (13,)
    out = oracle_preprocessing.normalize(x, landmarks)
    lo, hi = np.percentile(out.astype(np.float64), [1, 99])
    assert abs(lo) <= 1e-4 and abs(hi - 100) <= 1e-4, (lo, hi)
    masked = intensity_ref.train_landmarks_ref([x], masks=[x > x.mean()])
    out = oracle_preprocessing.normalize(x, masked, mask=x > x.mean())
    lo, hi = np.percentile(out[x > x.mean()].astype(np.float64), [1, 99])
    assert abs(lo) <= 1e-4 and abs(hi - 100) <= 1e-4, (lo, hi)


# ------------------------------------------------------------------------------------------------ the bound of the GPU suite
@pytest.mark.parametrize("name", list(intensity_ref.CASES))
def test_float32_mode_stays_inside_the_gpu_bound(name):
    """The bound of the GPU suite is 8 max(e32, 2^-23 max density), e32 the error of the float32 mode.  That bound means something only
    while e32 is what fp32 arithmetic must cost and no more: a term exp2(-d^2) matters up to |d| = 5.5 (beyond, it is below 1e-9),
    d is the difference of two values rounded to float32 of magnitude R = (range / h) sqrt(log2 e / 2) <= 64 at these sizes, so
    |delta d| <= 2^-24 (2 R + |d|) = 8e-6 and the term is off by at most 2 ln 2 |d| |delta d| = 6e-5 of itself, plus 256 x 2^-24 = 1.5e-5
    for its run: below 2^-13 of the largest density in all.  The float32 mode is held to that; and it is inside the GPU bound."""
    r = intensity_ref.case_refs(name)
    print("%s: e32 = %.3e, max density = %.3e, ratio %.3e" % (name, r["e32"], r["density"].max(), r["e32"] / r["density"].max()))
    assert np.isfinite(r["density"]).all() and r["density"].max() > 0
    assert r["e32"] <= 2.0 ** -13 * r["density"].max()
    assert r["e32"] <= r["bound"]
    n, _, _, m, _ = intensity_ref.CASES[name]
    assert np.array_equal(r["positions"], np.linspace(r["moments"][2], r["moments"][3], num=m))


@pytest.mark.parametrize("fault", intensity_ref.FAULTS)
def test_the_gpu_bound_sees_a_planted_mistake(fault):
    worst = 0.0
    for name in intensity_ref.SMALL_CASES:
        _, _, _, m, bw = intensity_ref.CASES[name]
        if m < 2 or (fault == "silverman_for_scott" and bw is not None):
            continue
        x, mask = intensity_ref.case_data(name)
        r = intensity_ref.case_refs(name)
        pos, bad = intensity_ref.kde_ref(x, m, bw_method=bw, mask=mask, float32=True, fault=fault)
        if fault == "step_over_m":
            assert not np.array_equal(pos, r["positions"])
        worst = max(worst, float(np.abs(bad - r["density"]).max()) / r["bound"])
    assert worst > 1.0, "%s stays inside the bound on every small case (worst %.3g of it)" % (fault, worst)


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_plan_and_workspace_queries_are_host_only():
    L = _lib.lib()
    out = (ctypes.c_int32 * 4)()
    for n, m in ((2, 100), (315, 1), (2849, 64), (2849, 65), (81 ** 3, 129), (1024 * 1024, 100), (1024 * 1024 + 1, 1024),
                 (129 ** 3, 3), (160 * 192 * 160, 100)):
        assert L.mri3d_kde_plan(n, 1, m, out) == 0
        assert tuple(out) == intensity_ref.kde_plan(n, m), (n, m)
    assert L.mri3d_kde_plan(160 * 192 * 160, 4, 100, out) == 0 and tuple(out) == (1024, 1024, 2, 5)
    for n, b, m in ((0, 1, 100), (-5, 1, 100), (100, 0, 100), (100, -1, 100), (100, 1, 0), (100, 1, 1025), (100, 1, -1)):
        assert L.mri3d_kde_plan(n, b, m, out) == EINVAL, (n, b, m)
        assert b"kde_plan" in L.mri3d_last_error()
    assert L.mri3d_kde_plan(100, 1, 100, None) == EINVAL
    q = L.mri3d_intensity_workspace_bytes
    assert q(160 * 192 * 160, 1, 100) == 1024 * 100 * 8 and q(160 * 192 * 160, 4, 100) == 4 * 1024 * 100 * 8
    assert q(160 * 192 * 160, 1, 0) == 1024 * 6 * 8 and q(2, 1, 1) == 6 * 8 and q(2849, 3, 100) == 3 * 3 * 100 * 8
    for n, b, m in ((0, 1, 100), (-5, 1, 100), (100, 0, 100), (100, 1, -1), (100, 1, 1025)):
        assert q(n, b, m) == 0, (n, b, m)


def _moments(x=A, mask=None, n=1000, batch=2, moments=C_, ws=D, ws_bytes=None):
    L = _lib.lib()
    if ws_bytes is None or ws_bytes == "one short":
        ws_bytes = L.mri3d_intensity_workspace_bytes(max(n, 1), max(batch, 1), 0) - (ws_bytes is not None)
    return L.mri3d_intensity_moments_f32(P(x), P(mask), n, batch, P(moments), P(ws), ws_bytes, None)


MOMENTS_BRANCHES = [
    ("NULL x", dict(x=None), EINVAL),
    ("NULL moments", dict(moments=None), EINVAL),
    ("n = 0", dict(n=0), EINVAL),
    ("n < 0", dict(n=-7), EINVAL),
    ("batch = 0", dict(batch=0), EINVAL),
    ("x off its element", dict(x=A + 2), EINVAL),
    ("moments off 8 bytes", dict(moments=C_ + 4), EINVAL),
    ("moments inside the workspace", dict(moments=D + 8), EINVAL),
    ("NULL workspace", dict(ws=None), EWORKSPACE),
    ("workspace one byte short", dict(ws_bytes="one short"), EWORKSPACE),
    ("workspace off 8 bytes", dict(ws=D + 4), EWORKSPACE),
]


@pytest.mark.parametrize("what,kw,code", MOMENTS_BRANCHES, ids=[b[0] for b in MOMENTS_BRANCHES])
def test_moments_validation(what, kw, code):
    assert _moments(**kw) == code, what
    msg = _lib.lib().mri3d_last_error()
    assert msg and b"intensity_moments" in msg, msg


def _kde(x=A, mask=None, n=1000, batch=2, moments=C_, positions=None, m=100, rule=0, scalar=0.0, pos_out=E, density=F, ws=D,
         ws_bytes=None):
    L = _lib.lib()
    if ws_bytes is None or ws_bytes == "one short":
        ws_bytes = L.mri3d_intensity_workspace_bytes(max(n, 1), max(batch, 1), min(max(m, 1), 1024)) - (ws_bytes is not None)
    return L.mri3d_kde_f32(P(x), P(mask), n, batch, P(moments), P(positions), m, rule, scalar, P(pos_out), P(density), P(ws), ws_bytes, None)


KDE_BRANCHES = [
    ("m = 0", dict(m=0), EINVAL),
    ("m = 1025", dict(m=1025), EINVAL),
    ("n < 0", dict(n=-1), EINVAL),
    ("n = 0", dict(n=0), EINVAL),
    ("batch = 0", dict(batch=0), EINVAL),
    ("unknown bandwidth rule", dict(rule=3), EINVAL),
    ("negative bandwidth rule", dict(rule=-1), EINVAL),
    ("factor 0", dict(rule=2, scalar=0.0), EINVAL),
    ("factor NaN", dict(rule=2, scalar=float("nan")), EINVAL),
    ("factor inf", dict(rule=2, scalar=float("inf")), EINVAL),
    ("NULL x", dict(x=None), EINVAL),
    ("NULL moments", dict(moments=None), EINVAL),
    ("NULL positions_out", dict(pos_out=None), EINVAL),
    ("NULL density", dict(density=None), EINVAL),
    ("density off 8 bytes", dict(density=F + 4), EINVAL),
    ("positions off 8 bytes", dict(positions=B + 4), EINVAL),
    ("density over positions_out", dict(density=E + 8), EINVAL),
    ("density inside the workspace", dict(density=D + 64), EINVAL),
    ("positions are the output", dict(positions=E), EINVAL),
    ("NULL workspace", dict(ws=None), EWORKSPACE),
    ("workspace one byte short", dict(ws_bytes="one short"), EWORKSPACE),
    ("workspace off 8 bytes", dict(ws=D + 4), EWORKSPACE),
]


@pytest.mark.parametrize("what,kw,code", KDE_BRANCHES, ids=[b[0] for b in KDE_BRANCHES])
def test_kde_validation(what, kw, code):
    assert _kde(**kw) == code, what
    msg = _lib.lib().mri3d_last_error()
    assert msg and b"kde" in msg, msg


# ------------------------------------------------------------------------------------------------ the Python layers
def test_cpu_tensors_have_no_fallback():
    x = torch.zeros(4, 4, 4)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        ops.intensity_moments(x)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        ops.gaussian_kde(x)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        intensity.intensity_histogram(x)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        intensity.histogram_table([x, x])
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        preprocessing.train_landmarks([x])
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        transforms.HistogramStandardization.train([{"MRI": x}], "MRI")


def test_argument_errors_need_no_device():
    with pytest.raises(ValueError, match="bw_method"):
        ops._bandwidth_rule("epanechnikov")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="positive and finite"):
            ops._bandwidth_rule(bad)
    assert ops._bandwidth_rule(None) == (0, 0.0) and ops._bandwidth_rule("scott") == (0, 0.0)
    assert ops._bandwidth_rule("silverman") == (1, 0.0) and ops._bandwidth_rule(0.3) == (2, 0.3)
    with pytest.raises(ValueError, match="no images"):
        preprocessing.train_landmarks([])
    with pytest.raises(ValueError, match="not both"):
        preprocessing.train_landmarks([torch.zeros(3)], mask=torch.ones(3), masking_function=transforms.ZNormalization.mean)
    with pytest.raises(ValueError, match="image_key"):
        transforms.HistogramStandardization.train([{"MRI": torch.zeros(3)}])
    with pytest.raises(ValueError, match="1 non-finite voxel among the 9 counted"):
        intensity._check_rows(np.array([[9, 1, 0, 1, 0.5, 0.1, 0, 0]]))
    with pytest.raises(ValueError, match="at least 2 counted voxels, got 1"):
        intensity._check_rows(np.array([[1, 0, 3, 3, 3, np.nan, 0, 0]]))
    with pytest.raises(ValueError, match=r"no variance .*volume 1"):
        intensity._check_rows(np.array([[9, 0, 0, 1, 0.5, 0.1, 0, 0], [9, 0, 3, 3, 3, 0.0, 0, 0]]))
