"""GPU suite of the tissue-class bias-field estimator: csrc/tissue.hip's two passes against the float64 restatement
(tests/tissue_ref.py) on the cases of tests/tissue_cases.py, and `tissue.segment` / `get_registered_img_bias_and_mask` end to end.

em_pass: per entry of the table |device - reference| <= (n 2^-52 + 2^-40) sum|terms|: two float64 summations of n terms in
different orders, and a few ulp on an exp argument of at most 745 with a 4x margin.  apply: restored and field within one fp32
ulp of the float64 reference rounded to fp32; labels bit-exact except where the reference's two best log-posteriors are closer
than 1e-9.  Every kernel-written buffer lies between guard bands, the workspace is pre-filled with 0xA5 and then 0xFF, and
every case runs twice to equal bits.

End to end (phantom (40, 48, 36), classes 3, order 3, 60 iterations): field rms error <= 0.01, label agreement >= 0.99,
coefficient of variation of the restored image over the true class 3 <= 0.05, and for seeds 0, 1 and 3 an order-0 run agrees on
<= 0.90 of the labels."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tissue_cases as TC
import tissue_ref as R
from guard import guarded
from mri_epilepsy_diagnosis_amd import _lib, ops, registration, tissue
from mri_epilepsy_diagnosis_amd.detection import preprocessing as det_pre

pytestmark = pytest.mark.gpu

RMS_MAX, AGREE_MIN, CV_MAX, ORDER0_AGREE_MAX = 0.01, 0.99, 0.05, 0.90


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---------------------------------------------------------------------------------------------- em_pass
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_em_pass_within_the_counted_bound_of_the_reference(name):
    shape, K, order, kind = TC.CASES[name]
    x, mask = TC.inputs(name)
    dx, dm = _dev(x), (_dev(mask) if mask is not None else None)
    L = _lib.lib()
    need = L.mri3d_tissue_em_workspace_bytes(*shape, K, order)
    plan = ops.tissue_em_plan(shape, K, order)
    assert need == plan["row_sums"] * plan["rows"] * 8
    entries = plan["entries"]
    ws = guarded(need, torch.uint8)                        # the region starts as 0xA5, the uint8 sentinel
    for it, (params, want, mag) in sorted(TC.reference(name).items()):
        p = np.ascontiguousarray(params, dtype=np.float64)
        got = []
        for fill in (0xA5, 0xFF, 0xFF):
            ws.region.fill_(fill)
            out = guarded(entries, torch.float64)
            rc = L.mri3d_tissue_em_pass(_p(dx), _p(dm), *shape, K, order, _hp(p), _p(out.region), _p(ws.region), need, None)
            assert rc == 0, L.mri3d_last_error()
            torch.cuda.synchronize()
            out.assert_guards_intact("%s sums" % name)
            ws.assert_guards_intact("%s workspace" % name)
            assert not bool(out.untouched().any())
            got.append(out.region.cpu().numpy().copy())
        assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()        # whatever the workspace held, and run to run
        err, lim = np.abs(got[0] - want), TC.bound(want[0], mag)
        worst = int(np.argmax(err / np.maximum(lim, 1e-300)))
        print("%s it %d: n %d, worst entry %d: |err| %.3g of bound %.3g" % (name, it, want[0], worst, err[worst], lim[worst]))
        assert got[0][0] == want[0]                                              # the count is exact
        assert np.isfinite(got[0]).all() and (err <= lim).all(), (name, it, worst, err[worst], lim[worst])
        if kind == "empty":
            assert (got[0] == 0).all()
        # the wrapper takes the same path through the shared workspace
        assert ops.tissue_em_pass(dx, dm, K, order, p).cpu().numpy().tobytes() == got[0].tobytes()


# ---------------------------------------------------------------------------------------------- apply
def _within_one_ulp(got, want64):
    want = want64.astype(np.float32)
    with np.errstate(all="ignore"):
        near = (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    return near | (np.isnan(got) & np.isnan(want))


@pytest.mark.parametrize("name", ["w37_odd_rows", "w64_full_step", "w65_one_lane", "w130_specials", "w1_two_trips", "order0_four"])
def test_apply_within_one_ulp_and_labels_exact_outside_near_ties(name):
    shape, K, order, kind = TC.CASES[name]
    x, mask = TC.inputs(name)
    dx, dm = _dev(x), (_dev(mask) if mask is not None else None)
    pi, mu, v, c = R.split(TC.reference(name)[5][0], K)
    params = np.concatenate([pi[::-1], mu[::-1], v[::-1], c])   # classes in reverse order: apply ranks them by their mean itself
    want_r, want_l, want_f, gap = R.apply(x, mask, K, order, params)
    sel = R.selected(x, mask)
    close = gap < 1e-9
    assert close.sum() <= 1e-3 * sel.sum()
    L = _lib.lib()
    p = np.ascontiguousarray(params)
    runs = []
    for _ in range(2):
        rest, lab, fld = guarded(shape, torch.float32), guarded(shape, torch.uint8), guarded(shape, torch.float32)
        rc = L.mri3d_tissue_apply(_p(dx), _p(dm), *shape, K, order, _hp(p), _p(rest.region), _p(lab.region), _p(fld.region), None)
        assert rc == 0, L.mri3d_last_error()
        torch.cuda.synchronize()
        for g, what in ((rest, "restored"), (lab, "labels"), (fld, "field")):
            g.assert_guards_intact("%s %s" % (name, what))
        assert not bool(rest.untouched().any()) and not bool(fld.untouched().any())
        runs.append((rest.region.cpu().numpy().copy(), lab.region.cpu().numpy().copy(), fld.region.cpu().numpy().copy()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    got_r, got_l, got_f = runs[0]
    assert _within_one_ulp(got_r, want_r).all() and _within_one_ulp(got_f, want_f).all()
    assert (got_l[~sel] == 0).all() and (got_l[~close] == want_l[~close]).all()
    assert got_l[sel].min() >= 1 and got_l.max() <= K
    # in place, without the field
    inplace, lab2 = guarded(shape, torch.float32), guarded(shape, torch.uint8)
    inplace.region.copy_(dx)
    rc = L.mri3d_tissue_apply(_p(inplace.region), _p(dm), *shape, K, order, _hp(p), _p(inplace.region), _p(lab2.region), None, None)
    assert rc == 0, L.mri3d_last_error()
    torch.cuda.synchronize()
    inplace.assert_guards_intact("%s restored in place" % name)
    lab2.assert_guards_intact("%s labels" % name)
    assert inplace.region.cpu().numpy().tobytes() == got_r.tobytes() and lab2.region.cpu().numpy().tobytes() == got_l.tobytes()
    # the wrapper
    wr, wl, wf = ops.tissue_apply(dx, dm, K, order, p, want_field=True)
    assert wr.cpu().numpy().tobytes() == got_r.tobytes() and wl.cpu().numpy().tobytes() == got_l.tobytes() and wf.cpu().numpy().tobytes() == got_f.tobytes()
    assert ops.tissue_apply(dx, dm, K, order, p)[2] is None


# ---------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _phantom(seed):
    return R.phantom(seed)


def _figures(seed, res):
    _x, mask, truth, P, _img = _phantom(seed)
    return R.end_to_end(res.restored.cpu().numpy(), res.labels.cpu().numpy(), res.field.cpu().numpy(), truth, P, mask)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_segment_meets_the_end_to_end_conditions(seed):
    x, mask, truth, P, _img = _phantom(seed)
    dx, dm = _dev(x), _dev(mask)
    res = tissue.segment(dx, dm, classes=3, order=3, iterations=60)
    rms, agree, cv = _figures(seed, res)
    ll = np.array(res.log_likelihood)
    print("seed %d: field rms %.4f, label agreement %.4f, CV over class 3 %.4f, smallest LL step %.3g" % (seed, rms, agree, cv, np.diff(ll).min()))
    assert rms <= RMS_MAX and agree >= AGREE_MIN and cv <= CV_MAX
    assert len(ll) == 60 and (np.diff(ll) >= -1e-9 * np.abs(ll).max()).all()
    assert res.selected == int((mask != 0).sum()) and list(res.means) == sorted(res.means)
    assert res.restored.dtype == torch.float32 and res.labels.dtype == torch.uint8 and res.field.shape == dx.shape
    head = mask != 0
    assert abs(np.log(res.field.cpu().numpy().astype(np.float64))[head].mean()) < 1e-6       # fp32 field, zero log-mean
    assert (res.labels.cpu().numpy()[~head] == 0).all()
    # the float64 restatement lands on the same estimate
    ref = R.segment(x, mask, 3, 3, 60)
    assert np.abs(res.coefficients - ref.coefficients).max() < 1e-4 and np.abs(res.means - ref.means).max() < 1e-4
    # deterministic end to end, and bias_correct is its restored image
    again = tissue.bias_correct(dx, mask=dm, classes=3, order=3, iterations=60)
    assert torch.equal(again, res.restored)
    if seed in (0, 1, 3):
        flat = tissue.segment(dx, dm, classes=3, order=0, iterations=60)
        agree0 = float(np.mean(flat.labels.cpu().numpy()[head] == truth[head]))
        print("seed %d: order 0 agrees on %.3f of the labels" % (seed, agree0))
        assert agree0 <= ORDER0_AGREE_MAX


def test_segment_refuses_too_few_voxels_and_bad_arguments():
    with pytest.raises(ValueError, match="fewer than"):
        tissue.segment(torch.ones(10, 10, 10, device="cuda"))                # 1000 < 100 * 20
    with pytest.raises(ValueError):
        tissue.segment(torch.ones(30, 30, 30, device="cuda"), classes=5)
    with pytest.raises(RuntimeError):
        tissue.segment(torch.ones(30, 30, 30, device="cuda"), mask=torch.ones(30, 30, 29, device="cuda"))


def test_get_registered_img_bias_and_mask_restores_a_shifted_phantom():
    seed = 1
    x, mask, truth, _P, img = _phantom(seed)
    shift = (1, -1, 1)                      # the phantom's outermost layer is background: nothing of the head wraps around
    moving, moving_mask = np.roll(x, shift, axis=(0, 1, 2)), np.roll(mask, shift, axis=(0, 1, 2))
    d_template, d_moving, d_mask = _dev(img), _dev(moving), _dev(moving_mask)
    kw = dict(dof=3, levels=2)
    registered, restored, reg_mask, matrix = det_pre.get_registered_img_bias_and_mask(d_moving, d_template, d_mask, **kw)
    want_img, want_mask = registration.apply(d_moving, matrix, x.shape, label=d_mask)
    assert torch.equal(registered, want_img) and torch.equal(reg_mask, want_mask) and reg_mask.dtype == torch.uint8
    assert matrix.shape == (3, 4) and restored.shape == d_template.shape and restored.dtype == torch.float32
    top = restored.cpu().numpy().astype(np.float64)[truth == 3]
    before = registered.cpu().numpy().astype(np.float64)[truth == 3]
    cv, cv_before = float(top.std() / top.mean()), float(before.std() / before.mean())
    print("translation found %s; CV over class 3 %.4f (%.4f before correction)" % (np.round(matrix[:, 3], 3), cv, cv_before))
    assert cv <= CV_MAX
    assert torch.equal(restored, tissue.bias_correct(registered, mask=reg_mask))
    # without a mask the estimate runs over every positive voxel, and tissue_kw reaches segment
    _r, restored2, none, _m = det_pre.get_registered_img_bias_and_mask(d_moving, d_template, None, tissue_kw=dict(iterations=5), **kw)
    assert none is None and restored2.shape == d_template.shape
