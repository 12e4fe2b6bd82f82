"""GPU suite of the intensity statistics (csrc/intensity.hip): per-volume moments, the Gaussian kernel density estimate, and their
wiring through ops, classification/intensity.py, preprocessing.train_landmarks and transforms.HistogramStandardization.train.

Launch plan of the KDE, as the cases below use it and assert it through mri3d_kde_plan (intensity.hip: kKdeTile, kIntMaxBlocks,
kde_slots): a row is cut into tiles of 1024 voxels, tile t goes to block t mod blocks, blocks = min(tiles, 1024) per row; a block is
4 waves, wave w evaluates voxels [256 w, 256 w + 256) of a tile; lane l owns positions l, l + 64, ... in slots = 1, 2, 4, 8 or 16
registers (the power of two >= ceil(m / 64)).
  2 voxels              one block, one tile with 2 voxels in wave 0 and 1022 that do not count
  5x7x9 = 315           one block, one partial tile: wave 1 ends inside its share, waves 2 and 3 see none
  7x11x37 = 2849        3 blocks, the last tile holds 801 voxels; odd, so rows 1 and 2 of a batch start off 16 bytes
  81^3 = 531 441        519 blocks of one tile each, the last with 1 voxel
  1024 x 1024 + 315     1025 tiles on 1024 blocks: the smallest row count of tiles whose loop goes round again (block 0 alone)
  129^3 = 2 146 689     2097 tiles on 1024 blocks: 3 trips for blocks 0..48, 2 for the rest (m = 3 keeps the reference cheap)
  m = 1, 2, 63, 64 | 65, 100, 128 | 129, 256 | 257, 512 | 513, 1024: both sides of every slots-per-lane boundary
The moments pass takes tiles of 4096 voxels, 16 per lane and trip, on min(tiles, 1024) blocks.

Checks.  count, non-finite count, min and max: exact.  Positions: the bits of np.linspace.  Mean against the two-pass float64 value:
64 x 2^-53 x sqrt(sum x^2 / count) (at least mean|x|), 64 a generous count of the additions on any voxel's path: 16 (a lane's trip) + trips (1 here)
+ 6 (wave) + 3 (waves) + 4 (a lane of the second stage) + 8 (its tree) = 38.  Variance: relative K x 2^-53 x (sum x^2 / count) /
variance with K = 128, not 64: the closing formula (Q - S^2 / n) / (n - 1) carries the error of S twice beside that of Q, 3 x 38
additions, and adds 3 roundings of its own; 117 rounded up.  Density: |device - float64| <= 8 max(e32, 2^-23 max density), e32 the
largest error of the float32 mode of tests/intensity_ref.py on that case (the convention of tests/test_mc_gpu.py and
tests/test_labels_gpu.py: the 8 covers the device's exp2 and another summation order)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import intensity_ref
from guard import guarded
from mri_epilepsy_diagnosis_amd import _lib, ops
from mri_epilepsy_diagnosis_amd.classification import intensity, preprocessing
from mri_epilepsy_diagnosis_amd.segmentation import transforms

pytestmark = pytest.mark.gpu

F64 = torch.float64
RULES = {None: (0, 0.0), "scott": (0, 0.0), "silverman": (1, 0.0)}
PLANS = {2: (1, 1), 315: (1, 1), 2849: (3, 1), 81 ** 3: (519, 1), 1024 * 1024 + 315: (1024, 2), 129 ** 3: (1024, 3)}   # n: (blocks, trips)
SLOTS = {1: 1, 2: 1, 3: 1, 28: 1, 63: 1, 64: 1, 65: 2, 100: 2, 128: 2, 129: 4, 256: 4, 257: 8, 512: 8, 513: 16, 1024: 16}
EPS = 2.0 ** -53


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(x, mask, m, bw=None, positions=None, garbage=None):
    """The two C entries on (B, n) rows with every kernel-written buffer between guard bands.  garbage: a value to fill workspace
    and outputs with first (None leaves the guards' own sentinel there).  Returns (moments, positions, density) on the host."""
    L = _lib.lib()
    b, n = x.shape
    rule, scalar = RULES[bw] if bw in RULES else (2, float(bw))
    need = L.mri3d_intensity_workspace_bytes(n, b, m)
    assert need >= L.mri3d_intensity_workspace_bytes(n, b, 0) > 0
    gm, gp, gd, gw = guarded((b, 8), F64), guarded((b, m), F64), guarded((b, m), F64), guarded(need, torch.uint8)
    if garbage is not None:
        for g in (gm, gp, gd):
            g.region.fill_(garbage)
        gw.region.view(F64).fill_(garbage)
    rc = L.mri3d_intensity_moments_f32(_p(x), _p(mask), n, b, _p(gm.region), _p(gw.region), need, _stream())
    assert rc == 0, L.mri3d_last_error()
    rc = L.mri3d_kde_f32(_p(x), _p(mask), n, b, _p(gm.region), _p(positions), m, rule, scalar, _p(gp.region), _p(gd.region),
                         _p(gw.region), need, _stream())
    assert rc == 0, L.mri3d_last_error()
    torch.cuda.synchronize()
    for g, what in ((gm, "moments"), (gp, "positions_out"), (gd, "density"), (gw, "workspace")):
        g.assert_guards_intact("%s, n = %d, m = %d" % (what, n, m))
    assert not bool(gm.untouched().any()) and not bool(gp.untouched().any()) and not bool(gd.untouched().any())
    return gm.region.cpu().numpy(), gp.region.cpu().numpy(), gd.region.cpu().numpy()


def _device_case(name, offset=0):
    """The case's row and mask on the device as (1, n) views that start `offset` elements into their buffers."""
    x, mask = intensity_ref.case_data(name)
    xd = torch.zeros(x.size + offset, dtype=torch.float32, device="cuda")
    xd[offset:] = torch.from_numpy(x).cuda()
    md = None
    if mask is not None:
        md = torch.ones(x.size + offset, dtype=torch.uint8, device="cuda")
        md[offset:] = torch.from_numpy(mask.astype(np.uint8)).cuda()
        md = md[offset:].view(1, -1)
    return xd[offset:].view(1, -1), md


def _assert_plan(n, m, batch=1):
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().mri3d_kde_plan(n, batch, m, out) == 0
    assert tuple(out) == (PLANS[n][0], 1024, SLOTS[m], PLANS[n][1]), (n, m, tuple(out))
    assert tuple(out) == intensity_ref.kde_plan(n, m)


def _assert_moments(got, want, what):
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3], (what, got, want)
    assert got[6] == 0 and got[7] == 0
    mean_err, var_err = abs(got[4] - want[4]), abs(got[5] - want[5])
    mean_sq = want[5] * (want[0] - 1) / want[0] + want[4] ** 2          # sum x^2 / count
    print("%s: mean off %.3e (bound %.3e), variance off %.3e (bound %.3e)"
          % (what, mean_err, 64 * EPS * np.sqrt(mean_sq), var_err, 128 * EPS * mean_sq))
    assert mean_err <= 64 * EPS * np.sqrt(mean_sq), what               # mean|x| <= sqrt(mean x^2)
    assert var_err <= 128 * EPS * mean_sq, what


def _assert_density(got_pos, got, name, what):
    r = intensity_ref.case_refs(name)
    err = float(np.abs(got - r["density"]).max())
    print("%s: density off %.3e, bound %.3e (e32 %.3e, max density %.3e)" % (what, err, r["bound"], r["e32"], r["density"].max()))
    assert np.array_equal(got_pos, r["positions"]), what                # np.linspace, bit for bit
    assert np.isfinite(got).all() and err <= r["bound"], what


def _reference(x, m, bw, mask, positions=None):
    """(positions, float64 density, the density bound) of a row that is no case of intensity_ref.CASES."""
    pos, want = intensity_ref.kde_ref(x, m, positions=positions, bw_method=bw, mask=mask)
    _, d32 = intensity_ref.kde_ref(x, m, positions=positions, bw_method=bw, mask=mask, float32=True)
    return pos, want, 8 * max(float(np.abs(d32 - want).max()), 2.0 ** -23 * float(want.max()))


# ------------------------------------------------------------------------------------------------ the C entries
@pytest.mark.parametrize("name", list(intensity_ref.CASES))
def test_moments_positions_and_density(name):
    n, _, _, m, bw = intensity_ref.CASES[name]
    _assert_plan(n, m)
    x, mask = _device_case(name)
    mom, pos, den = _run(x, mask, m, bw)
    _assert_moments(mom[0], intensity_ref.case_refs(name)["moments"], name)
    _assert_density(pos[0], den[0], name, name)
    # the same bits again, whatever the workspace and the outputs held
    for garbage in (0.0, 1.0e300, float("nan")):
        mom2, pos2, den2 = _run(x, mask, m, bw, garbage=garbage)
        for a, b in ((mom, mom2), (pos, pos2), (den, den2)):
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), (name, garbage)


@pytest.mark.parametrize("name", ["blocks_t1", "blocks_scanner_masked", "one_tile_masked"])
def test_rows_off_their_alignment_leave_the_same_bits(name):
    """x 4-byte and mask 1-byte aligned only (views one element into their buffers, odd n): the scalar tile path, and the very bits
    of the aligned call, since a voxel's lane and turn follow from its index in the row alone."""
    n, _, _, m, bw = intensity_ref.CASES[name]
    assert n % 2 == 1
    x0, mask0 = _device_case(name)
    x1, mask1 = _device_case(name, offset=1)
    assert x0.data_ptr() % 16 == 0 and x1.data_ptr() % 16 == 4 and (mask1 is None or mask1.data_ptr() % 4 == 1)
    want = _run(x0, mask0, m, bw)
    got = _run(x1, mask1, m, bw)
    for a, b in zip(want, got):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    _assert_density(got[1][0], got[2][0], name, name + " off alignment")


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_a_batch_is_its_rows(masked):
    """B = 3 rows of 2849 voxels (rows 1 and 2 start 4 and 8 bytes off a 16-byte boundary) against three B = 1 calls: bit-equal."""
    n, m = 2849, 100
    _assert_plan(n, m, batch=3)
    rows = np.stack([intensity_ref.t1_like(70 + k, (n,)) * np.float32(1 + 9 * k) for k in range(3)])
    x = torch.from_numpy(rows).cuda()
    mask = None
    if masked:
        mask = torch.from_numpy(np.stack([r > r.mean() for r in rows]).astype(np.uint8)).cuda()
    mom, pos, den = _run(x, mask, m, "silverman")
    for k in range(3):
        one = _run(x[k].clone().view(1, -1), None if mask is None else mask[k].clone().view(1, -1), m, "silverman")
        for a, b in zip((mom, pos, den), one):
            assert np.array_equal(a[k].view(np.int64), b[0].view(np.int64)), k
        want_pos, want, bound = _reference(rows[k], m, "silverman", rows[k] > rows[k].mean() if masked else None)
        assert np.array_equal(pos[k], want_pos) and np.abs(den[k] - want).max() <= bound, k
    assert not np.array_equal(den[0], den[1])


def test_given_positions_are_shared_by_the_rows():
    name = "blocks_scanner_silverman"
    x, _ = _device_case(name)
    xs = torch.cat([x, x * 0.5])
    want_pos = np.linspace(-100.0, 20000.0, 77)
    positions = torch.from_numpy(want_pos).cuda()
    _, pos, den = _run(xs, None, 77, 0.3, positions=positions)
    rows = xs.cpu().numpy()
    for k in range(2):
        _, want, bound = _reference(rows[k], None, 0.3, None, positions=want_pos)
        assert np.array_equal(pos[k], want_pos) and np.abs(den[k] - want).max() <= bound, k
    got_pos, got = ops.gaussian_kde(xs, positions=positions, bw_method=0.3)
    assert np.array_equal(got.cpu().numpy().view(np.int64), den.view(np.int64)) and np.array_equal(got_pos.cpu().numpy(), pos)


DEGENERATE = ["no voxel counts", "one voxel counts", "constant volume", "one NaN voxel", "one Inf voxel"]


def _degenerate(what):
    x = torch.from_numpy(intensity_ref.t1_like(5, (2849,))).cuda()
    mask = None
    if what == "no voxel counts":
        mask = torch.zeros(2849, dtype=torch.bool, device="cuda")
    elif what == "one voxel counts":
        mask = torch.zeros(2849, dtype=torch.bool, device="cuda")
        mask[1500] = True
    elif what == "constant volume":
        x.fill_(5.3)
    elif what == "one NaN voxel":
        x[2000] = float("nan")
    else:
        x[7] = float("-inf")
    return x, mask


@pytest.mark.parametrize("what", DEGENERATE)
def test_rows_without_a_density_end_in_nan_and_a_value_error(what):
    """Inputs scipy has no answer for, in a batch beside a row that has one: the kernels write NaN densities for that row alone, and
    the Python layer turns the moments row into a ValueError."""
    x, mask = _degenerate(what)
    good = torch.from_numpy(intensity_ref.t1_like(6, (2849,))).cuda()
    rows = torch.stack([x, good])
    masks = None if mask is None else torch.stack([mask, torch.ones_like(mask)]).view(torch.uint8)
    mom, pos, den = _run(rows, masks, 100)
    assert np.isnan(den[0]).all(), what
    alone = _run(good.view(1, -1), None, 100)
    assert np.isfinite(den[1]).all() and np.array_equal(den[1], alone[2][0]) and np.array_equal(mom[1], alone[0][0])
    want_mom = intensity_ref.moments_ref(x.cpu().numpy(), None if mask is None else mask.cpu().numpy())
    assert np.array_equal(mom[0][:4], want_mom[:4]), (mom[0], want_mom)
    if what == "constant volume":
        assert mom[0][5] == 0.0 and abs(mom[0][4] - np.float32(5.3)) <= 64 * EPS * 5.3
    text = {"no voxel counts": "at least 2 counted voxels, got 0", "one voxel counts": "at least 2 counted voxels, got 1",
            "constant volume": "no variance", "one NaN voxel": "1 non-finite voxel among the 2849 counted",
            "one Inf voxel": "1 non-finite voxel among the 2849 counted"}[what]
    with pytest.raises(ValueError, match=text):
        intensity.intensity_histogram(x.view(7, 11, 37), mask=None if mask is None else mask.view(7, 11, 37))
    with pytest.raises(ValueError, match=r"volume 0"):
        intensity.histogram_table([x, good], masks=None if mask is None else [mask, torch.ones_like(mask)])


# ------------------------------------------------------------------------------------------------ the Python layers
def test_ops_and_histogram_functions():
    name = "blocks_t1"
    n, _, _, m, _ = intensity_ref.CASES[name]
    x, _ = _device_case(name)
    vol = x.view(7, 11, 37)
    r = intensity_ref.case_refs(name)
    mom = ops.intensity_moments(x)
    assert mom.shape == (1, 8) and mom.dtype == F64 and mom.is_cuda
    _assert_moments(mom[0].cpu().numpy(), r["moments"], "ops.intensity_moments")
    pos, den = ops.gaussian_kde(x, num_positions=m)
    assert pos.shape == den.shape == (1, m) and den.dtype == F64 and den.is_cuda
    _assert_density(pos[0].cpu().numpy(), den[0].cpu().numpy(), name, "ops.gaussian_kde")
    hp, hd = intensity.intensity_histogram(vol)
    assert isinstance(hd, np.ndarray) and np.array_equal(hd, den[0].cpu().numpy()) and np.array_equal(hp, r["positions"])
    keep = vol > vol.mean()
    mp, md = intensity.intensity_histogram(vol, 65, mask=keep, bw_method="silverman")
    want_pos, want, bound = _reference(vol.cpu().numpy(), 65, "silverman", keep.cpu().numpy())
    assert np.array_equal(mp, want_pos) and np.abs(md - want).max() <= bound
    tp, td = intensity.histogram_table([vol, vol * 2.0, vol[:5]])                    # two sizes: one by one
    assert tp.shape == td.shape == (3, 100) and np.array_equal(td[0], hd)
    bp, bd = intensity.histogram_table(torch.stack([vol, vol * 2.0]))                # one size: one batch
    assert np.array_equal(bd, td[:2]) and np.array_equal(bp, tp[:2])


def _landmark_volumes():
    shapes = ((7, 11, 37), (12, 10, 9), (16, 16, 16))
    return [intensity_ref.t1_like(90 + k, s) * np.float32(1 + 4 * k) + np.float32(3 * k) for k, s in enumerate(shapes)]


@pytest.mark.parametrize("masking", [None, "mean"])
def test_train_landmarks_is_the_reference(masking, tmp_path):
    arrays = _landmark_volumes()
    tensors = [torch.from_numpy(a).cuda() for a in arrays]
    fn = transforms.ZNormalization.mean if masking else None
    # the masks of the reference are those the masking function gives on the device: the comparison is of the landmarks
    masks = [fn(t).cpu().numpy() for t in tensors] if masking else None
    want = intensity_ref.train_landmarks_ref(arrays, masks=masks)
    path = os.path.join(str(tmp_path), "landmarks.npy")
    got = preprocessing.train_landmarks(tensors, masking_function=fn, output_path=path)
    assert got.dtype == np.float64 and got.shape == (13,)
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert np.array_equal(np.load(path), want)
    if masking:
        given = preprocessing.train_landmarks(tensors, mask=[torch.from_numpy(k).cuda() for k in masks])
        assert np.array_equal(given, want)
    subjects = [{"MRI": t, "LABEL": torch.zeros_like(t)} for t in tensors]
    trained = transforms.HistogramStandardization.train(subjects, "MRI", masking_function=fn)
    assert np.array_equal(trained, want)
    assert np.array_equal(transforms.HistogramStandardization.train(tensors, masking_function=fn), want)
    stage = transforms.HistogramStandardization(landmarks_dict={"MRI": trained})
    assert np.array_equal(stage.landmarks_dict["MRI"], want)
    other = intensity_ref.train_landmarks_ref(arrays, cutoff=(0.05, 0.95), masks=masks)
    assert np.array_equal(preprocessing.train_landmarks(tensors, cutoff=(0.05, 0.95), masking_function=fn), other)
    assert not np.array_equal(other, want)


def test_trained_landmarks_standardise_their_own_volume():
    """normalize with the landmarks of one volume sends that volume's 1st / 99th percentile to 0 / 100 (float32 output: 1e-4, as in
    tests/test_intensity.py)."""
    t = torch.from_numpy(intensity_ref.t1_like(11, (12, 14, 16))).cuda()
    out = preprocessing.normalize(t, preprocessing.train_landmarks([t]))
    lo, hi = np.percentile(out.cpu().numpy().astype(np.float64), [1, 99])
    assert abs(lo) <= 1e-4 and abs(hi - 100) <= 1e-4, (lo, hi)
