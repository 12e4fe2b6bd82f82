"""GPU suite of the tissue classes with a Potts prior: mri3d_tissue_mrf_pass against the float64 restatement
(tests/tissue_mrf_ref.py) on the cases of tests/tissue_mrf_cases.py, and `tissue.segment(beta=...)` end to end.

mrf_pass: per entry of the table |device - reference| <= tissue_mrf_ref.bound, the family's (n 2^-52 + 2^-40) sum|terms| with
the roundings of beta n_k and of the normaliser counted the same way; labels_out exact except where the reference's two best
logt lie within 2^-30 max|logt| of each other; at beta = 0 the table is within the family's bound of `ops.tissue_em_pass` on the
same inputs.  labels_out, sums and the workspace lie between guard bands, the workspace and labels_out start as 0xA5, and every
pass runs twice to equal bits.  The whole family (`em_pass`, `mrf_pass`, `apply`) reproduces the digests of
tests/golden/tissue_family_bits.json, entry for entry.

End to end (phantom (40, 48, 36) with noise 0.10, classes 3, order 3, 60 iterations, warmup 20, beta 1): label agreement >= 0.98,
field rms error <= 0.007, isolated voxels <= 100; the three figures equal the reference's to four decimals and the labels differ
from the reference's on at most 10^-4 of the selected voxels."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import tissue_bits
import tissue_cases as TC
import tissue_mrf_cases as MC
import tissue_mrf_ref as M
import tissue_ref as R
from guard import guarded
from mri_epilepsy_diagnosis_amd import _lib, ops, tissue
from mri_epilepsy_diagnosis_amd.detection import preprocessing as det_pre

pytestmark = pytest.mark.gpu

AGREE_MIN, RMS_MAX, ISOLATED_MAX = 0.98, 0.007, 100
LABEL_SHARE_MAX = 1e-4
BITS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tissue_family_bits.json")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---------------------------------------------------------------------------------------------- mrf_pass
@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_mrf_pass_table_within_the_counted_bound_and_labels_exact_off_near_ties(name):
    shape, K, order, kind = MC.CASES[name]
    x, mask = MC.inputs(name)
    dx, dm = _dev(x), (_dev(mask) if mask is not None else None)
    L = _lib.lib()
    need = L.mri3d_tissue_em_workspace_bytes(*shape, K, order)
    entries = ops.tissue_table_size(K, order)
    ws = guarded(need, torch.uint8)
    used, plain = 0.0, {}
    for it, beta, mode, params, labels_in, want in MC.reference(name):
        p = np.ascontiguousarray(params, dtype=np.float64)
        dl = _dev(labels_in) if labels_in is not None else None
        runs = []
        for _ in range(2):
            ws.region.fill_(0xA5)
            out, lab = guarded(entries, torch.float64), guarded(shape, torch.uint8)      # the label region starts as 0xA5
            rc = L.mri3d_tissue_mrf_pass(_p(dx), _p(dm), *shape, K, order, _hp(p), beta, mode, _p(dl), _p(lab.region), _p(out.region),
                                         _p(ws.region), need, None)
            assert rc == 0, L.mri3d_last_error()
            torch.cuda.synchronize()
            out.assert_guards_intact("%s sums" % name)
            lab.assert_guards_intact("%s labels_out" % name)
            ws.assert_guards_intact("%s workspace" % name)
            assert not bool(out.untouched().any())
            runs.append((out.region.cpu().numpy().copy(), lab.region.cpu().numpy().copy()))
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
        got, got_l = runs[0]
        what = (name, it, beta, mode)
        # the table
        err, lim = np.abs(got - want.sums), M.bound(want.sums[0], want.mag, beta)
        frac = err / np.maximum(lim, 1e-300)
        worst = int(np.argmax(frac))
        used = max(used, float(frac[worst]))
        assert got[0] == want.sums[0], what                                          # the count is exact
        assert np.isfinite(got).all() and (err <= lim).all(), what + (worst, err[worst], lim[worst])
        # the labels: every voxel written, zeros where unselected (a wave step of background included), exact off the near-ties
        sel = want.selected
        assert (got_l[~sel] == 0).all(), what
        off = ~M.near_ties(want)
        assert np.array_equal(got_l[off], want.labels[off]), what + (int((got_l[off] != want.labels[off]).sum()),)
        if kind == "empty":
            assert (got == 0).all() and (got_l == 0).all()
        if beta == 0.0:
            # the plain pass on the same inputs, within the family's bound of its reference
            if it not in plain:
                plain[it] = (ops.tissue_em_pass(dx, dm, K, order, p).cpu().numpy(), R.em_sums(x, mask, K, order, params))
            em, (ref, mag) = plain[it]
            assert (np.abs(got - em) <= TC.bound(ref[0], mag)).all(), what
            assert (np.abs(got - ref) <= TC.bound(ref[0], mag)).all(), what
        # the wrapper takes the same path through the shared workspace
        w_sums, w_lab = ops.tissue_mrf_pass(dx, dm, K, order, p, beta, mode, dl)
        assert w_sums.cpu().numpy().tobytes() == got.tobytes() and w_lab.cpu().numpy().tobytes() == got_l.tobytes()
    print("%s: worst used fraction of the table bound %.3g" % (name, used))


def test_overlapping_label_buffers_are_refused_and_leave_the_output_untouched():
    name = "w37_odd_rows"
    shape, K, order, _kind = MC.CASES[name]
    x, mask = MC.inputs(name)
    dx, dm = _dev(x), _dev(mask)
    it, beta, mode, params, labels_in, _want = MC.reference(name)[1]
    both = guarded(shape, torch.uint8)
    both.region.copy_(_dev(labels_in))
    before = both.region.clone()
    with pytest.raises(_lib.Mri3dError, match="labels_in and labels_out overlap"):
        ops.tissue_mrf_pass(dx, dm, K, order, params, beta, mode, both.region, both.region)
    n = int(np.prod(shape))
    long = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.Mri3dError, match="labels_in and labels_out overlap"):
        ops.tissue_mrf_pass(dx, dm, K, order, params, beta, mode, long[:n].view(shape), long[8:].view(shape))
    with pytest.raises(_lib.Mri3dError, match="labels_in is null"):
        ops.tissue_mrf_pass(dx, dm, K, order, params, beta, mode, None)
    torch.cuda.synchronize()
    assert torch.equal(both.region, before)
    both.assert_guards_intact("refused labels")


def test_the_family_reproduces_its_recorded_bits():
    """tests/golden/tissue_family_bits.json (tools/record_tissue_bits.py): the sha256 of every output of `em_pass`, `mrf_pass` and `apply` on
    the parity cases and on a sweep over all 12 (classes, order) instances, as the toolchain the file names compiled them.  A change of
    csrc/tissue.hip that is meant to keep the arithmetic keeps every entry."""
    with open(BITS_FILE) as f:
        want = json.load(f)["entries"]
    got = tissue_bits.device_bits(ops)
    assert sorted(got) == sorted(want)
    bad = sorted(name for name in want if got[name] != want[name])
    assert not bad, (len(bad), bad[:20])


# ---------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _phantom(seed):
    return M.phantom(seed, 0.10)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_segment_with_the_prior_meets_the_end_to_end_conditions_and_matches_the_reference(seed):
    x, mask, truth, P, _img = _phantom(seed)
    dx, dm = _dev(x), _dev(mask)
    res = tissue.segment(dx, dm, classes=3, order=3, iterations=60, beta=1.0, warmup=20)
    labels = res.labels.cpu().numpy()

    class Host:
        pass
    host = Host()
    host.restored, host.labels, host.field = res.restored.cpu().numpy(), labels, res.field.cpu().numpy()
    agree, rms, isolated = M.figures(host, truth, P, mask)
    ref = M.segment(x, mask, 3, 3, 60, beta=1.0, warmup=20)
    r_agree, r_rms, r_isolated = M.figures(ref, truth, P, mask)
    head = mask != 0
    share = float(np.mean(labels[head] != ref.labels[head]))
    print("seed %d: agreement %.4f (reference %.4f), field rms %.4f (%.4f), isolated %d (%d), labels differing from the reference's %.3g"
          % (seed, agree, r_agree, rms, r_rms, isolated, r_isolated, share))
    assert agree >= AGREE_MIN and rms <= RMS_MAX and isolated <= ISOLATED_MAX
    assert abs(agree - r_agree) <= 0.5e-4 and abs(rms - r_rms) <= 0.5e-4 and isolated == r_isolated       # to four decimals
    assert share <= LABEL_SHARE_MAX
    assert res.labels.dtype == torch.uint8 and res.labels.shape == dx.shape and (labels[~head] == 0).all()
    assert labels[head].min() >= 1 and labels.max() <= 3 and list(res.means) == sorted(res.means)
    assert len(res.log_likelihood) == 60 and res.selected == int(head.sum())
    assert np.abs(res.coefficients - ref.coefficients).max() < 1e-4 and np.abs(res.means - ref.means).max() < 1e-4
    # the same bits run to run, and bias_correct passes the prior through
    assert torch.equal(tissue.bias_correct(dx, mask=dm, classes=3, order=3, iterations=60, beta=1.0, warmup=20), res.restored)


def test_segment_with_beta_zero_is_the_plain_segment_bit_for_bit_and_launches_no_prior_kernel():
    from guard import kernels_launched
    x, mask, _truth, _P, _img = _phantom(0)
    dx, dm = _dev(x), _dev(mask)
    want = tissue.segment(dx, dm, classes=3, order=3, iterations=12)
    got, names = kernels_launched(lambda: tissue.segment(dx, dm, classes=3, order=3, iterations=12, beta=0.0, warmup=5))
    assert not any("mrf" in n for n in names) and any("tissue_em_rows" in n for n in names)
    for a, b in zip(want, got):
        if torch.is_tensor(a):
            assert torch.equal(a, b)
        else:
            assert np.array_equal(np.asarray(a), np.asarray(b))
    _res, names = kernels_launched(lambda: tissue.segment(dx, dm, classes=3, order=3, iterations=12, beta=1.0, warmup=5))
    assert any("tissue_mrf_rows" in n for n in names)
    for kw in (dict(warmup=12), dict(warmup=-1), dict(beta=-1.0), dict(beta=9.0)):
        with pytest.raises(ValueError):
            tissue.segment(dx, dm, classes=3, order=3, iterations=12, **dict(dict(beta=1.0, warmup=5), **kw))


def test_get_registered_img_bias_and_mask_takes_the_prior_through_tissue_kw():
    x, mask, truth, _P, img = R.phantom(1)
    shift = (1, -1, 1)                      # the phantom's outermost layer is background: nothing of the head wraps around
    moving, moving_mask = np.roll(x, shift, axis=(0, 1, 2)), np.roll(mask, shift, axis=(0, 1, 2))
    d_template, d_moving, d_mask = _dev(img), _dev(moving), _dev(moving_mask)
    registered, restored, reg_mask, matrix = det_pre.get_registered_img_bias_and_mask(d_moving, d_template, d_mask, tissue_kw=dict(beta=1.0),
                                                                                      dof=3, levels=2)
    assert restored.shape == d_template.shape and restored.dtype == torch.float32
    assert torch.equal(restored, tissue.bias_correct(registered, mask=reg_mask, beta=1.0))
    top = restored.cpu().numpy().astype(np.float64)[truth == 3]
    cv = float(top.std() / top.mean())
    print("CV over class 3 with the prior %.4f" % cv)
    assert cv <= 0.05                       # the existing condition of the plain path on this phantom
