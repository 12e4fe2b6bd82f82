"""CPU suite of the cross-entropy / focal references (tests/ce_ref.py) and of segmentation/losses.py's host side: the reference
is F.cross_entropy at gamma = 0, its closed-form gradient is autograd's, nothing counting gives 0, the class-weight rules, and the
float32 emulation of the kernel's expressions stays inside the GPU suite's bound on every row of tests/ce_cases.py while each of
a list of planted mistakes leaves it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ce_cases
import ce_ref
from ce_cases import CASES, case_id
from mri_epilepsy_diagnosis_amd.segmentation import losses

F64 = torch.float64
SMALL = ce_cases.SMALL
EMULATED = [c for c in CASES if c.spatial in (ce_cases.SMALL, ce_cases.TRIPS)]       # the cubes of bwd_trips repeat their arithmetic


def _torch_ce(z, lab, w, C):
    t = lab.long().clone()
    t[t >= C] = -100
    return F.cross_entropy(z, t, weight=w, ignore_index=-100, reduction="mean")


@pytest.mark.parametrize("weights", ["none", "random", "zero_one"])
@pytest.mark.parametrize("kind", ["mixed", "ignored", "sample_ignored"])
@pytest.mark.parametrize("C", [2, 5, 32])
def test_gamma_zero_is_torch_cross_entropy(C, kind, weights):
    z = (3.0 * torch.randn(2, C, *SMALL, generator=torch.Generator().manual_seed(C))).double()
    lab, w = ce_cases.class_map_of(kind, C, SMALL, 10 + C), ce_cases.weights_of(weights, C, 20 + C)
    w64 = None if w is None else w.double()
    zr = z.clone().requires_grad_(True)
    want = _torch_ce(zr, lab, w64, C)
    want.backward()
    got, grad = ce_ref.ce_ref(z, lab, w64)
    assert abs(got.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    assert (grad - zr.grad).abs().max().item() <= 1e-15


@pytest.mark.parametrize("scale", [3.0, 32.0])
@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, 3.5])
@pytest.mark.parametrize("C", [2, 5, 32])
def test_closed_form_gradient_is_autograd(C, gamma, scale):
    z = (scale * torch.randn(2, C, *SMALL, generator=torch.Generator().manual_seed(30 + C))).double()
    lab, w = ce_cases.class_map_of("ignored", C, SMALL, 40 + C), ce_cases.weights_of("zero_one", C, 50 + C).double()
    _, auto = ce_ref.ce_ref(z, lab, w, gamma)
    closed = ce_ref.ce_grad_closed(z, lab, w, gamma)
    assert bool(torch.isfinite(closed).all())
    assert (auto - closed).abs().max().item() <= 1e-15, (auto - closed).abs().max().item()


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_nothing_counting_gives_zero_and_a_zero_gradient(gamma):
    C = 5
    z = torch.randn(2, C, *SMALL, generator=torch.Generator().manual_seed(60)).double()
    ignored = ce_cases.class_map_of("all_ignored", C, SMALL, 61)
    assert int((ignored < C).sum()) == 0
    only_two = torch.full((2,) + SMALL, 2, dtype=torch.uint8)
    w = torch.ones(C, dtype=F64)
    w[2] = 0.0                                                  # every class that occurs has weight 0
    for lab, weight in ((ignored, None), (only_two, w)):
        for fn in (lambda: ce_ref.ce_ref(z, lab, weight, gamma), lambda: ce_ref.emulate(z.float(), lab, weight, gamma)):
            loss, grad = fn()
            assert float(loss) == 0.0 and bool((grad == 0).all())
        assert bool((ce_ref.ce_grad_closed(z, lab, weight, gamma) == 0).all())
    # the Dice part is untouched by that: the compound is dice_weight * Dice
    import labels_ref
    loss, grad = ce_ref.compound_ref(z, ignored, 0.7, 1.3, None, gamma)
    dl, dg = labels_ref.dice_index_ref(z, ignored)
    assert abs(loss.item() - 0.7 * dl.item()) <= 1e-15 and (grad - 0.7 * dg).abs().max().item() <= 1e-18


def test_class_weight_rules_on_a_hand_made_histogram():
    counts = [100, 0, 25, 400]
    inv = losses.weights_from_counts(counts, "inverse")
    want = np.array([1 / 100, 0, 1 / 25, 1 / 400])
    assert np.allclose(inv, want / want[[0, 2, 3]].mean(), rtol=1e-6) and inv[1] == 0 and inv.dtype == np.float32
    sq = losses.weights_from_counts(counts, "inverse_sqrt")
    want = np.array([1 / 10, 0, 1 / 5, 1 / 20])
    assert np.allclose(sq, want / want[[0, 2, 3]].mean(), rtol=1e-6)
    med = losses.weights_from_counts(counts, "median")                # median of (100, 25, 400) = 100: 1, 4, 0.25 before the mean
    assert np.allclose(med, np.array([1, 0, 4, 0.25]) / 1.75, rtol=1e-6)
    for rule in losses.RULES:
        w = losses.weights_from_counts(counts, rule)
        assert abs(w[[0, 2, 3]].mean() - 1) <= 1e-6 and w[1] == 0
        assert np.all(losses.weights_from_counts([0, 0, 0], rule) == 0)
    assert np.allclose(losses.weights_from_counts([7, 7, 7], "inverse"), 1.0)
    with pytest.raises(ValueError):
        losses.weights_from_counts(counts, "balanced")


@pytest.fixture(scope="module")
def references():
    """case -> (inputs, float64 loss, float64 gradient, e32), computed once for the two tests below."""
    cache = {}

    def get(c):
        k = case_id(c)
        if k not in cache:
            z, lab, w = ce_cases.inputs_of(c)
            cache[k] = (z, lab, w) + ce_ref.reference(z, lab, w, c.gamma, c.dice_weight, c.ce_weight)
        return cache[k]
    return get


@pytest.mark.parametrize("c", EMULATED, ids=case_id)
def test_the_kernels_expressions_in_float32_stay_inside_the_bound(c, references):
    z, lab, w, l64, g64, e32 = references(c)
    loss, grad = ce_ref.emulate(z, lab, w, c.gamma, c.dice_weight, c.ce_weight)
    ok, lerr, worst, finite = ce_ref.inside(loss, grad, l64, g64, e32, c.dtype)
    assert ok, "loss error %.2e, gradient error %.2f x its bound, finite %s" % (lerr, worst, finite)
    if c.kind == "all_ignored" and c.dice_weight == 0.0:
        assert float(loss) == 0.0 and bool((grad.float() == 0).all())


# a planted mistake must show on the rows that can see it: which rows those are
SEES = {
    "count_denominator": lambda c: c.weights in ("random", "zero_one") and c.kind not in ("all_ignored",),
    "weight_missing_in_gradient": lambda c: c.weights in ("random", "zero_one") and c.kind not in ("all_ignored",),
    "gamma_term_dropped": lambda c: c.gamma > 0 and c.kind != "all_ignored" and c.scale == 3.0,
    "ignored_counted": lambda c: c.kind in ("ignored", "sample_ignored", "all_ignored") and c.scale == 3.0,
    "log_pt": lambda c: c.scale == 32.0,
    "weights_swapped": lambda c: c.dice_weight > 0 and c.kind != "all_ignored",
}


@pytest.mark.parametrize("mistake", ce_ref.MISTAKES)
def test_a_planted_mistake_leaves_the_bound(mistake, references):
    rows = [c for c in EMULATED if SEES[mistake](c) and c.group != "pitched"]
    assert len(rows) >= 4, mistake
    missed = []
    for c in rows:
        z, lab, w, l64, g64, e32 = references(c)
        loss, grad = ce_ref.emulate(z, lab, w, c.gamma, c.dice_weight, c.ce_weight, mistake=mistake)
        if ce_ref.inside(loss, grad, l64, g64, e32, c.dtype)[0]:
            missed.append(case_id(c))
    assert not missed, "%s passes on %s" % (mistake, missed)
