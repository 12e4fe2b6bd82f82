"""CPU suite of the float64 restatement of the tissue classes with a Potts prior (tests/tissue_mrf_ref.py): beta = 0 is the plain
pass, the label rule of a pass, the order of the passes in `segment`, the end-to-end conditions with and without the prior,
planted mistakes that the GPU suite's comparisons or an end-to-end condition must see, and the near-ties of the GPU parity cases.

End-to-end conditions (phantom (40, 48, 36), seeds 0..3, classes 3, order 3, 60 iterations, warmup 20); "isolated" counts the
selected voxels whose label none of their six neighbours shares:
    noise 0.10, beta 1:  label agreement >= 0.98, field rms error <= 0.007, isolated voxels <= 100
    noise 0.10, beta 0:  label agreement <= 0.94, field rms error >= 0.009, isolated voxels >= 800   (the prior is what does it)
    noise 0.04, beta 1:  field rms error <= 0.0025, label agreement >= 0.999
Measured with this reference: 0.9881-0.9902 / 0.0028-0.0049 / 40-53; 0.9276-0.9319 / 0.0100-0.0145 / 1067-1131;
0.0011-0.0019 / 1.0000."""
import functools

import numpy as np
import pytest

import tissue_mrf_cases as MC
import tissue_mrf_ref as M
import tissue_ref as R

AGREE_MIN, RMS_MAX, ISOLATED_MAX = 0.98, 0.007, 100
PLAIN_AGREE_MAX, PLAIN_RMS_MIN, PLAIN_ISOLATED_MIN = 0.94, 0.009, 800
CLEAN_RMS_MAX, CLEAN_AGREE_MIN = 0.0025, 0.999
NEAR_TIE_SHARE = 1e-3


@functools.lru_cache(maxsize=None)
def _phantom(seed, noise):
    return M.phantom(seed, noise)


@functools.lru_cache(maxsize=None)
def _run(seed, noise, beta):
    x, mask, _truth, _P, _img = _phantom(seed, noise)
    return M.segment(x, mask, classes=3, order=3, iterations=60, beta=beta, warmup=20)


def _figures(seed, noise, res):
    _x, mask, truth, P, _img = _phantom(seed, noise)
    return M.figures(res, truth, P, mask)


def test_the_phantom_at_noise_004_is_tissue_refs():
    for a, b in zip(R.phantom(2), M.phantom(2)):
        assert np.array_equal(a, b)
    assert not np.array_equal(M.phantom(2, 0.10)[0], R.phantom(2)[0])


@pytest.mark.parametrize("name", ["w37_odd_rows", "w130_specials", "w65_one_lane", "d1_no_depth_neighbour"])
def test_beta_zero_reproduces_the_plain_pass_for_any_labels(name):
    shape, K, order, _kind = MC.CASES[name]
    x, mask = MC.inputs(name)
    params = MC.parameters(name)[5]
    want, _mag = R.em_sums(x, mask, K, order, params)
    labels = np.random.default_rng(3).integers(0, 256, shape).astype(np.uint8)
    for mode, L in ((0, labels), (1, labels), (2, None)):
        got = M.mrf_pass(x, mask, K, order, params, 0.0, mode, L).sums
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", ["w37_odd_rows", "w130_specials", "h1_no_height_neighbour"])
def test_a_pass_leaves_the_resting_colour_and_zeroes_the_unselected(name):
    shape, K, order, _kind = MC.CASES[name]
    x, mask = MC.inputs(name)
    sel = R.selected(x, mask)
    d, h, w = np.indices(shape)
    colour = (d + h + w) & 1
    seen_change = False
    for it, beta, mode, params, L, res in MC.reference(name):
        assert (res.labels[~sel] == 0).all() and res.labels[sel].min() >= (0 if mode != 2 else 1)
        if mode == 2:
            assert res.labels[sel].max() <= K
            continue
        rest = sel & (colour != mode)
        assert np.array_equal(res.labels[rest], L[rest])               # garbage bytes included: copied as they are
        active = sel & (colour == mode)
        assert res.labels[active].min() >= 1 and res.labels[active].max() <= K
        seen_change = seen_change or bool((res.labels[active] != L[active]).any())
    assert seen_change


def test_neighbour_counts_stop_at_the_border_and_ignore_bytes_outside_the_classes():
    L = np.zeros((3, 4, 5), dtype=np.uint8)
    L[0, 0, 0], L[2, 3, 4], L[1, 1, 1], L[1, 1, 2] = 1, 1, 2, 200
    n = M.neighbour_counts(L, 3)
    assert n.sum() == 3 + 3 + 6 and n[0, 2, 3, 3] == 1 and n[0, 0, 0, 4] == 0 and n[0, 2, 0, 0] == 0      # no wrap-around
    assert n[1, 1, 1, 0] == 1 and n[1, 1, 1, 2] == 1 and n[2].sum() == 0
    assert M.neighbour_counts(L, 3, "neighbour_wrap")[0, 2, 0, 0] == 1
    assert M.neighbour_counts(L, 3, "zero_counts_as_class")[0, 1, 2, 3] == 6


def test_segment_runs_warm_up_start_colours_and_two_closing_half_sweeps_in_that_order():
    x, mask, _t, _P, _i = _phantom(0, 0.10)
    seen = []
    M.segment(x, mask, 3, 1, iterations=9, beta=1.0, warmup=4, hook=seen.append)
    assert seen == ["em"] * 4 + [2] + [1, 0, 1, 0] + [0, 1]            # t = 5..8 are modes t & 1, then the closing pair
    seen = []
    M.segment(x, mask, 3, 1, iterations=3, beta=1.0, warmup=0, hook=seen.append)
    assert seen == [2, 1, 0, 0, 1]
    seen = []
    plain = M.segment(x, mask, 3, 1, iterations=5, beta=0.0, warmup=2, hook=seen.append)
    assert seen == ["em"] * 5
    want = R.segment(x, mask, 3, 1, 5)
    assert np.array_equal(plain.labels, want.labels) and np.array_equal(plain.field, want.field)
    for warmup in (-1, 5):
        with pytest.raises(ValueError):
            M.segment(x, mask, 3, 1, iterations=5, beta=1.0, warmup=warmup)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_prior_meets_the_end_to_end_conditions_and_the_plain_mixture_does_not(seed):
    res = _run(seed, 0.10, 1.0)
    agree, rms, isolated = _figures(seed, 0.10, res)
    print("seed %d, noise 0.10, beta 1: agreement %.4f, field rms %.4f, isolated %d" % (seed, agree, rms, isolated))
    assert agree >= AGREE_MIN and rms <= RMS_MAX and isolated <= ISOLATED_MAX
    assert len(res.log_likelihood) == 60 and list(res.means) == sorted(res.means)
    mask = _phantom(seed, 0.10)[1]
    assert (res.labels[mask == 0] == 0).all() and res.labels[mask != 0].min() >= 1 and res.labels.max() <= 3
    assert abs(np.log(res.field)[mask != 0].mean()) < 1e-12
    agree0, rms0, isolated0 = _figures(seed, 0.10, _run(seed, 0.10, 0.0))
    print("seed %d, noise 0.10, beta 0: agreement %.4f, field rms %.4f, isolated %d" % (seed, agree0, rms0, isolated0))
    assert agree0 <= PLAIN_AGREE_MAX and rms0 >= PLAIN_RMS_MIN and isolated0 >= PLAIN_ISOLATED_MIN


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_prior_leaves_the_clean_phantoms_as_they_were(seed):
    agree, rms, isolated = _figures(seed, 0.04, _run(seed, 0.04, 1.0))
    print("seed %d, noise 0.04, beta 1: agreement %.4f, field rms %.4f, isolated %d" % (seed, agree, rms, isolated))
    assert rms <= CLEAN_RMS_MAX and agree >= CLEAN_AGREE_MIN


# ------------------------------------------------------------------------------------------ planted mistakes
def _seen_by_the_pass_comparisons(name, mistake):
    """Whether a device pass with the mistake would fail the GPU suite's label comparison or its table bound on this case."""
    shape, K, order, _kind = MC.CASES[name]
    x, mask = MC.inputs(name)
    labels = table = False
    for it, beta, mode, params, L, want in MC.reference(name):
        wrong = M.mrf_pass(x, mask, K, order, params, beta, mode, L, mistake=mistake)
        off = ~M.near_ties(want)
        labels = labels or bool((wrong.labels[off] != want.labels[off]).any())
        table = table or bool((np.abs(wrong.sums - want.sums) > M.bound(want.sums[0], want.mag, beta)).any())
    return labels, table


@pytest.mark.parametrize("mistake,name", [("colour_flipped", "w37_odd_rows"), ("synchronous", "w37_odd_rows"), ("neighbour_wrap", "w64_full_step"),
                                          ("zero_counts_as_class", "w130_specials"), ("no_normaliser", "w65_one_lane")])
def test_planted_mistakes_break_the_label_comparison_or_the_table_bound(mistake, name):
    labels, table = _seen_by_the_pass_comparisons(name, mistake)
    print("%s on %s: labels differ %s, table outside the bound %s" % (mistake, name, labels, table))
    assert labels or table
    if mistake in ("colour_flipped", "synchronous"):
        assert labels
    if mistake == "no_normaliser":
        assert table and not labels


def test_labels_left_in_the_order_of_the_parameters_fail_the_agreement():
    seed, K = 0, 3
    x, mask, truth, P, _img = _phantom(seed, 0.10)
    res = _run(seed, 0.10, 1.0)
    # the same estimate with its classes in descending order of their mean
    pi, mu, v, c = R.split(res.raw_params, K)
    params = np.concatenate([pi[::-1], mu[::-1], v[::-1], c])
    raw = np.where(res.raw_labels > 0, K + 1 - res.raw_labels, 0).astype(np.uint8)
    good = M.label_table(params, K)[raw]
    assert np.array_equal(good, res.labels)
    wrong = M.label_table(params, K, mistake="labels_unsorted")[raw]
    head = mask != 0
    agree = float(np.mean(wrong[head] == truth[head]))
    print("labels_unsorted: agreement %.4f" % agree)
    assert agree < AGREE_MIN


# ------------------------------------------------------------------------------------------ what the GPU cases cover
def test_the_parity_cases_cover_what_they_promise():
    shapes = [c[0] for c in MC.CASES.values()]
    assert {1, 3, 37, 64, 65, 130} <= {s[2] for s in shapes}
    assert any(s[0] == 1 for s in shapes) and any(s[1] == 1 for s in shapes)
    assert any(s[0] * s[1] == 35 for s in shapes)
    assert {c[1] for c in MC.CASES.values()} == {2, 3, 4} and {0, 3} <= {c[2] for c in MC.CASES.values()}
    assert {None, "rows", "empty", "specials"} <= {c[3] for c in MC.CASES.values()}
    assert set(MC.BETAS) == {0.0, 0.5, 2.0} and MC.ITERATIONS == (0, 5)
    for name, c in MC.CASES.items():
        assert int(np.prod(c[0])) <= 10 ** 5
    it, beta, mode, params, L, _res = MC.reference("w37_odd_rows")[1]
    assert mode == 0 and 0.01 < np.mean(L == 0) and 0.01 < np.mean(L == 200) < 0.06


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_near_ties_of_the_parity_cases_are_rare(name):
    worst = 0.0
    for it, beta, mode, params, L, res in MC.reference(name):
        n = int(res.selected.sum())
        share = float(M.near_ties(res).sum()) / max(n, 1)
        worst = max(worst, share)
    print("%s: largest share of near-ties %.3g" % (name, worst))
    assert worst <= NEAR_TIE_SHARE
