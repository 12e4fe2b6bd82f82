"""The host loop of the tissue-class bias-field estimator: an EM whose every iteration is one streaming pass of
csrc/tissue.hip over the volume (`ops.tissue_em_pass`, or `ops.tissue_mrf_pass` with the Potts prior on the labels, beta > 0) and a few float64 operations on the
table it returns.  The device counterpart of the FAST call in the reference's detection/preprocessing_utils.py:11-53 (`_restore`,
the bias-corrected image); no partial volumes, no spline field.  tests/tissue_ref.py and tests/tissue_mrf_ref.py restate the
algorithm in float64 numpy."""
import collections

import numpy as np
import torch

from .. import ops
from ..classification.preprocessing import percentile

MIN_VOXELS_PER_TERM = 100
VARIANCE_FLOOR = 1e-6      # of the initial class variance

TissueSegmentation = collections.namedtuple(
    "TissueSegmentation", ["restored", "labels", "field", "means", "variances", "priors", "coefficients", "log_likelihood", "selected"])


def _exponents(order):
    return [(i, j, k) for i in range(order + 1) for j in range(order + 1 - i) for k in range(order + 1 - i - j)]


def _update(params, sums, classes, order, v_floor):
    """The M-step from one pass's table: class means, variances and priors, and the non-constant field coefficients from the
    normal equations A c = g, A[n, n'] = Mw[e_n + e_n'], g[n] = Mt[e_n].  The constant stays 0: the class means carry it."""
    K, M = classes, ops.tissue_coefficients(order)
    pi, mu, v, c = params[:K].copy(), params[K:2 * K].copy(), params[2 * K:3 * K].copy(), params[3 * K:].copy()
    s0, s1, s2 = sums[2:2 + K], sums[2 + K:2 + 2 * K], sums[2 + 2 * K:2 + 3 * K]
    for k in range(K):
        if s0[k] >= 1.0:
            mu[k] = s1[k] / s0[k]
            v[k] = max(s2[k] / s0[k] - mu[k] * mu[k], v_floor)
    pi = s0 / s0.sum()
    if M > 1:
        ex, ex2 = _exponents(order), _exponents(2 * order)
        where = {e: n for n, e in enumerate(ex2)}
        mw = sums[2 + 3 * K:2 + 3 * K + len(ex2)]
        g = sums[2 + 3 * K + len(ex2):]
        A = np.array([[mw[where[(a[0] + b[0], a[1] + b[1], a[2] + b[2])]] for b in ex] for a in ex])
        c = np.concatenate([[0.0], np.linalg.solve(A[1:, 1:], g[1:])])
    return np.concatenate([pi, mu, v, c])


def segment(volume, mask=None, classes=3, order=3, iterations=60, beta=0.0, warmup=20):
    """Estimate tissue classes and the bias field of a (d, h, w) device volume: a TissueSegmentation with
        restored        volume * exp(-b), float32, every voxel
        labels          uint8: 0 where the voxel is not selected, else 1..classes by ascending class mean
        field           exp(b), float32; its logarithm has zero mean over the selected voxels
        means, variances, priors    of the classes on log(restored), ascending by mean (float64 numpy)
        coefficients    of b, np.linspace(-1, 1, N) coordinates, `ops`' bias-field nesting (what `transforms.bias_field` takes)
        log_likelihood  one value per iteration, of the parameters that iteration started from
        selected        the voxels that counted: mask non-zero (no mask: all), finite and > 0
    classes 2..4, order 0..3.  Only the sums table of a pass crosses to the host per iteration.
    beta > 0 (at most 8) puts a Markov random field prior on the labels, beta per face neighbour of the same class (hidden-MRF EM with
    red-black ICM): iterations t < warmup are plain passes, iteration `warmup` starts the label volume, later ones
    update the colour t & 1 of it, and two closing half-sweeps with the final parameters give `labels`.  The warm-up is needed:
    the prior from the first iteration merges classes.  0 <= warmup < iterations.  beta = 0 is the plain mixture and ignores warmup."""
    if not torch.is_tensor(volume) or not volume.is_cuda or volume.dim() != 3:
        raise RuntimeError("tissue.segment: volume must be a (d, h, w) ROCm device tensor (got %s); there is no CPU fallback"
                           % (getattr(volume, "device", type(volume)),))
    if mask is not None and (not torch.is_tensor(mask) or not mask.is_cuda or tuple(mask.shape) != tuple(volume.shape)):
        raise RuntimeError("tissue.segment: mask must be a device tensor of the volume's shape %s" % (tuple(volume.shape),))
    K, order, iterations, beta, warmup = int(classes), int(order), int(iterations), float(beta), int(warmup)
    if not 2 <= K <= 4 or not 0 <= order <= 3:
        raise ValueError("tissue.segment: classes must be 2..4 and order 0..3, got %d and %d" % (K, order))
    if not 0.0 <= beta <= 8.0:
        raise ValueError("tissue.segment: beta must be in 0..8, got %g" % beta)
    if beta > 0 and not 0 <= warmup < iterations:      # without the prior the warm-up is the whole run, whatever it says
        raise ValueError("tissue.segment: warmup must be in 0..iterations - 1 = %d, got %d" % (iterations - 1, warmup))
    x = volume.to(torch.float32).contiguous()
    if mask is not None:
        mask = (mask != 0).contiguous()
    M = ops.tissue_coefficients(order)
    sel = torch.isfinite(x) & (x > 0)
    if mask is not None:
        sel &= mask
    n_sel = int(sel.sum())
    if n_sel < MIN_VOXELS_PER_TERM * M:
        raise ValueError("tissue.segment: %d selected voxels, fewer than %d per field term (%d)" % (n_sel, MIN_VOXELS_PER_TERM, MIN_VOXELS_PER_TERM * M))
    y = torch.log(x[sel].double()).float()
    pct = percentile(y, [5.0, 95.0] + [100.0 * (2 * k + 1) / (2 * K) for k in range(K)])
    v0 = ((pct[1] - pct[0]) / (2 * K)) ** 2
    if not v0 > 0:
        raise ValueError("tissue.segment: the 5th and 95th percentile of the log-intensities coincide (%g)" % pct[0])
    params = np.concatenate([np.full(K, 1.0 / K), pct[2:], np.full(K, v0), np.zeros(M)])
    sums_dev = torch.empty(ops.tissue_table_size(K, order), dtype=torch.float64, device=x.device)
    log_likelihood = []
    prior = beta > 0
    cur, nxt = (torch.empty(x.shape, dtype=torch.uint8, device=x.device) for _ in range(2)) if prior else (None, None)
    for t in range(iterations):
        if not prior or t < warmup:
            ops.tissue_em_pass(x, mask, K, order, params, out=sums_dev)
        else:   # the start pass, then one colour per iteration; `cur` holds the labels the next pass reads
            ops.tissue_mrf_pass(x, mask, K, order, params, beta, 2 if t == warmup else t & 1, None if t == warmup else cur, nxt, out=sums_dev)
            cur, nxt = nxt, cur
        sums = sums_dev.cpu().numpy()
        log_likelihood.append(float(sums[1]))
        params = _update(params, sums, K, order, VARIANCE_FLOOR * v0)
    if prior:   # both colours once more with the parameters the last M-step left
        for mode in (0, 1):
            ops.tissue_mrf_pass(x, mask, K, order, params, beta, mode, cur, nxt, out=sums_dev)
            cur, nxt = nxt, cur
    # the field's mean over the selected voxels from the moments of 1: a pass with every v = 1 has w = sum_k p_k = 1
    ones = np.concatenate([params[:2 * K], np.ones(K), np.zeros(M)])
    m1 = ops.tissue_em_pass(x, mask, K, order, ones, out=sums_dev).cpu().numpy()[2 + 3 * K:]
    ex2 = _exponents(2 * order)
    c = params[3 * K:].copy()
    mean_b = float(sum(cn * m1[ex2.index(e)] for cn, e in zip(c, _exponents(order))) / n_sel)
    c[0] -= mean_b
    idx = np.argsort(params[K:2 * K], kind="stable")
    pi, mu, v = params[:K][idx], params[K:2 * K][idx] + mean_b, params[2 * K:3 * K][idx]
    restored, labels, field = ops.tissue_apply(x, mask, K, order, np.concatenate([pi, mu, v, c]), want_field=True)
    if prior:   # the prior's labels, in the order of `params`, renumbered by ascending mean
        lut = np.zeros(K + 1, dtype=np.uint8)
        lut[1 + idx] = 1 + np.arange(K)
        labels = ops.remap_labels(cur, torch.from_numpy(lut).to(x.device), out=cur)
    return TissueSegmentation(restored, labels, field, mu, v, pi, c, log_likelihood, n_sel)


def bias_correct(volume, **kw):
    """The bias-corrected volume alone (`segment(volume, **kw).restored`)."""
    return segment(volume, **kw).restored
