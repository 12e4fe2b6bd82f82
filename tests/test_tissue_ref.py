"""CPU suite of the tissue-class bias-field estimator's float64 restatement (tests/tissue_ref.py): the moment table against
the explicit basis, a log-likelihood that never decreases, the end-to-end conditions on the four phantoms, and planted mistakes
that the parity bound or an end-to-end condition must see.

End-to-end conditions (classes 3, order 3, 60 iterations, phantom (40, 48, 36), seeds 0..3): rms over the head of
(b - mean b) - (P - mean P) <= 0.01; label agreement >= 0.99; coefficient of variation of the restored image over the true
class 3 <= 0.05; for seeds 0, 1 and 3 the same run at order 0 agrees on <= 0.90 of the labels."""
import functools

import numpy as np
import pytest

import tissue_cases as TC
import tissue_ref as R

RMS_MAX, AGREE_MIN, CV_MAX, ORDER0_AGREE_MAX = 0.01, 0.99, 0.05, 0.90


@functools.lru_cache(maxsize=None)
def _phantom(seed):
    return R.phantom(seed)


@functools.lru_cache(maxsize=None)
def _run(seed, order=3, mistake=None):
    x, mask, _truth, _P, _img = _phantom(seed)
    return R.segment(x, mask, classes=3, order=order, iterations=60, mistake=mistake)


def _conditions(seed, res):
    _x, mask, truth, P, _img = _phantom(seed)
    return R.end_to_end(res.restored, res.labels, res.field, truth, P, mask)


def _meets(figures):
    rms, agree, cv = figures
    return rms <= RMS_MAX and agree >= AGREE_MIN and cv <= CV_MAX


@pytest.mark.parametrize("shape", [(6, 5, 7), (5, 1, 9), (1, 6, 4)])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_moment_table_assembles_the_gram_matrix_of_the_explicit_basis(shape, order):
    rng = np.random.default_rng(order)
    x = rng.uniform(0.2, 1.5, shape).astype(np.float32)
    mask = (rng.uniform(size=shape) < 0.8).astype(np.uint8)
    K = 3
    params = np.concatenate([[0.2, 0.3, 0.5], [-1.0, -0.4, 0.2], [0.05, 0.03, 0.04], rng.uniform(-0.2, 0.2, R.ncoef(order))])
    sums, _ = R.em_sums(x, mask, K, order, params)
    A, g = R.normal_equations(sums, K, order)
    # the same two from the basis written out voxel by voxel
    pi, mu, v, c = R.split(params, K)
    xh, yh, zh = R.coordinates(shape)
    sel = R.selected(x, mask)
    idx = np.argwhere(sel)
    phi = np.stack([xh[idx[:, 0]] ** i * yh[idx[:, 1]] ** j * zh[idx[:, 2]] ** k for i, j, k in R.exponents(order)], axis=1)
    y = np.log(x[sel].astype(np.float64))
    r = y - phi @ c
    logt = np.log(pi) - 0.5 * np.log(v) - (r[:, None] - mu) ** 2 / (2 * v)
    p = np.exp(logt - logt.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    w = (p / v).sum(axis=1)
    t = (p * (y[:, None] - mu) / v).sum(axis=1)
    np.testing.assert_allclose(A, phi.T @ (w[:, None] * phi), rtol=1e-12, atol=1e-12 * np.abs(A).max())
    np.testing.assert_allclose(g, phi.T @ t, rtol=1e-12, atol=1e-12 * np.abs(phi.T * t).sum(axis=1).max())
    assert sums[0] == sel.sum() and len(sums) == R.table_size(K, order)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_log_likelihood_never_decreases_and_the_reference_meets_the_conditions(seed):
    res = _run(seed)
    ll = np.array(res.log_likelihood)
    figures = _conditions(seed, res)
    A, _g = R.normal_equations(R.em_sums(*_phantom(seed)[:2], 3, 3, res.trace[-1])[0], 3, 3)
    print("seed %d: field rms %.4f, label agreement %.4f, CV over class 3 %.4f, smallest LL step %.3g, cond(A) %.3g"
          % ((seed,) + figures + (np.diff(ll).min(), np.linalg.cond(A[1:, 1:]))))
    assert len(ll) == 60 and (np.diff(ll) >= 0).all()
    assert figures[0] <= RMS_MAX and figures[1] >= AGREE_MIN and figures[2] <= CV_MAX
    assert list(res.means) == sorted(res.means)
    x, mask = _phantom(seed)[:2]
    head = mask != 0
    assert abs(np.log(res.field)[head].mean()) < 1e-12                      # zero log-mean over the selected voxels
    assert (res.labels[~head] == 0).all() and res.labels[head].min() >= 1
    assert np.mean(res.gap[head] < 1e-9) <= 1e-3                            # what the device's labels may differ on


@pytest.mark.parametrize("seed", [0, 1, 3])
def test_a_constant_field_does_not_meet_the_label_condition(seed):
    truth, mask = _phantom(seed)[2], _phantom(seed)[1]
    agree = float(np.mean(_run(seed, order=0).labels[mask != 0] == truth[mask != 0]))
    print("seed %d: order 0 agrees on %.3f of the labels" % (seed, agree))
    assert agree <= ORDER0_AGREE_MAX


def test_too_few_selected_voxels_is_an_error_before_any_iteration():
    x = np.ones((10, 10, 10), dtype=np.float32)
    with pytest.raises(ValueError):
        R.segment(x, None, order=3)            # 1000 < 100 * 20


@pytest.mark.parametrize("mistake", ["w_no_inv_v", "t_from_r", "moment_exponent"])
def test_planted_mistakes_in_the_sums_break_the_parity_bound(mistake):
    """What a device pass with the same mistake would show against the correct reference."""
    name = "w37_odd_rows"
    shape, K, order, _kind = TC.CASES[name]
    x, mask = TC.inputs(name)
    params, sums, mag = TC.reference(name)[5]
    wrong, _ = R.em_sums(x, mask, K, order, params, mistake=mistake)
    over = np.abs(wrong - sums) > TC.bound(sums[0], mag)
    assert over.any()
    assert not over[:2 + 3 * K].any()          # the class sums do not depend on w, t or the exponents


@pytest.mark.parametrize("mistake", ["w_no_inv_v", "t_from_r", "moment_exponent", "labels_unsorted"])
def test_planted_mistakes_fail_an_end_to_end_condition(mistake):
    seed = 0
    x, mask, truth, P, _img = _phantom(seed)
    if mistake == "labels_unsorted":
        # classes that the EM leaves in descending order of their mean: the labels come out reversed
        res = _run(seed)
        params = np.concatenate([res.priors[::-1], res.means[::-1], res.variances[::-1], res.coefficients])
        restored, labels, field, _gap = R.apply(x, mask, 3, 3, params, mistake=mistake)
        figures = R.end_to_end(restored, labels, field, truth, P, mask)
        good = R.apply(x, mask, 3, 3, params)
        assert _meets(R.end_to_end(good[0], good[1], good[2], truth, P, mask))
    else:
        try:
            with np.errstate(all="ignore"):                                     # a broken run may overflow on its way
                figures = _conditions(seed, _run(seed, mistake=mistake))
        except (np.linalg.LinAlgError, FloatingPointError, ValueError):
            return                                                              # the run did not even finish
    print("%s: field rms %.4f, label agreement %.4f, CV %.4f" % ((mistake,) + figures))
    assert not _meets(figures)
