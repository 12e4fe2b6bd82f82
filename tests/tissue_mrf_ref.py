"""float64 numpy restatement of the tissue classes with a Potts prior on the labels (mri3d_tissue_mrf_pass in csrc/tissue.hip,
`tissue.segment(beta=..., warmup=...)`), on top of tests/tissue_ref.py.

State: a uint8 label volume L, 0 where a voxel is not selected, else 1 + its class in the order of `params`.  n_k(i) counts the
face neighbours of voxel i inside the volume whose L_in is k + 1 (bytes outside 1..K count for no class).  Per selected voxel
    logt_k = log pi_k - log(v_k)/2 - log(2 pi)/2 - (r - mu_k)^2 / (2 v_k) + beta n_k,    p_k = softmax_k logt_k,
    new = 1 + argmax_k logt_k (the first of equal maxima),
and the sums table is tissue_ref.em_sums' with these p_k, entry [1] the pseudo-log-likelihood
    sum_i [logsumexp_k logt_k - log sum_k pi_k exp(beta n_k)].
mode 0 / 1: the voxels with (d + h + w) & 1 == mode take `new`, the selected others keep L_in; mode 2: no neighbour term, L_in is
not read, every selected voxel takes `new`.

`mistake` plants one error (tests/test_tissue_mrf_ref.py shows that the suite's conditions see each): 'colour_flipped',
'synchronous', 'neighbour_wrap', 'zero_counts_as_class', 'no_normaliser', 'labels_unsorted'."""
import numpy as np

import tissue_ref as R

MISTAKES = ("colour_flipped", "synchronous", "neighbour_wrap", "zero_counts_as_class", "no_normaliser", "labels_unsorted")
BETA_MAX = 8.0


def phantom(seed, noise=0.04, shape=R.PHANTOM_SHAPE):
    """tissue_ref.phantom with the noise's standard deviation as a parameter (0.04 gives that phantom's bits)."""
    d, h, w = np.meshgrid(*(np.linspace(-1, 1, n) for n in shape), indexing="ij")
    s = np.sin(7 * d + 1 + 2 * np.sin(3 * h)) * np.cos(6 * h + 0.5) + np.sin(8 * w + 2 + 3 * d) * np.cos(5 * d - 1) + 0.7 * np.sin(9 * h * w + 4 * d)
    head = d * d + h * h + w * w < 0.97 ** 2
    q = np.quantile(s[head], [0.2, 0.6])
    truth = np.where(head, 1 + (s > q[0]) + (s > q[1]), 0).astype(np.uint8)
    img = np.asarray(R.CLASS_INTENSITY)[np.maximum(truth, 1) - 1] + noise * np.random.default_rng(seed).standard_normal(shape)
    img = np.where(head, np.maximum(img, 1e-3), 0.0)
    coef = np.random.default_rng(100 + seed).uniform(-0.5, 0.5, 20)
    coef[0] = 0.0
    P = R.field_log(shape, coef, 3)
    return (img * np.exp(P)).astype(np.float32), head.astype(np.uint8), truth, P, img.astype(np.float32)


def neighbour_counts(labels, classes, mistake=None):
    """n[k, d, h, w]: how many of the up to six face neighbours inside the volume hold k + 1."""
    L = np.asarray(labels, dtype=np.uint8)
    n = np.zeros((classes,) + L.shape, dtype=np.int64)
    for k in range(classes):
        is_k = L == k + 1
        if mistake == "zero_counts_as_class" and k == 0:
            is_k = is_k | (L == 0)
        for axis in range(3):
            for step in (1, -1):
                moved = np.roll(is_k, step, axis=axis)
                if mistake != "neighbour_wrap":
                    edge = [slice(None)] * 3
                    edge[axis] = 0 if step == 1 else -1
                    moved[tuple(edge)] = False
                n[k] += moved
    return n


class Pass:
    """What one pass returns: sums, magnitudes (the sums of the absolute values of each entry's terms), labels, and per voxel the
    gap between the two best logt and the largest |logt| (inf / 0 where the voxel is not selected)."""


def mrf_pass(x, mask, classes, order, params, beta, mode, labels_in, mistake=None):
    K = classes
    x = np.asarray(x)
    if not (np.isfinite(beta) and 0.0 <= beta <= BETA_MAX) or mode not in (0, 1, 2):
        raise ValueError("tissue_mrf_ref: beta %r or mode %r" % (beta, mode))
    pi, mu, v, c = R.split(params, K)
    sel = R.selected(x, mask)
    y = np.zeros(x.shape)
    y[sel] = np.log(x[sel].astype(np.float64))
    r = y - R.field_log(x.shape, c, order)
    if mode == 2:
        n = np.zeros((K,) + x.shape, dtype=np.int64)
        L_in = np.zeros(x.shape, dtype=np.uint8)
    else:
        L_in = np.asarray(labels_in, dtype=np.uint8)
        n = neighbour_counts(L_in, K, mistake)
    bn = float(beta) * n.astype(np.float64)
    with np.errstate(divide="ignore"):
        plain = (np.log(pi) - 0.5 * np.log(v) - 0.5 * R.LOG_2PI)[:, None, None, None] - (r[None] - mu[:, None, None, None]) ** 2 / (2.0 * v[:, None, None, None])
    logt = plain + bn
    lmax = logt.max(axis=0)
    e = np.exp(logt - lmax[None])
    s = e.sum(axis=0)
    p = e / s[None] * sel[None]
    lse = (lmax + np.log(s)) * sel
    norm = np.log((pi[:, None, None, None] * np.exp(bn)).sum(axis=0)) * sel
    if mistake == "no_normaliser":
        norm = np.zeros(x.shape)
    ll = lse - norm
    w = (p / v[:, None, None, None]).sum(axis=0)
    t = (p * ((y[None] - mu[:, None, None, None]) / v[:, None, None, None])).sum(axis=0)
    out, mag = [], []
    for absolute, dst in ((False, out), (True, mag)):
        a = np.abs if absolute else (lambda z: z)
        dst += [a(sel.astype(np.float64)).sum(), (np.abs(lse) + np.abs(norm)).sum() if absolute else ll.sum()]
        dst += list(a(p).sum(axis=(1, 2, 3))) + list(a(p * r[None]).sum(axis=(1, 2, 3))) + list(a(p * (r * r)[None]).sum(axis=(1, 2, 3)))
        dst += list(R._moments(w, x.shape, 2 * order, absolute)) + list(R._moments(t, x.shape, order, absolute))
    new = (1 + np.argmax(logt, axis=0)).astype(np.uint8)
    d, h, ww = np.indices(x.shape)
    colour = (d + h + ww) & 1
    if mode == 2 or mistake == "synchronous":
        active = np.ones(x.shape, dtype=bool)
    else:
        active = colour == ((1 - mode) if mistake == "colour_flipped" else mode)
    res = Pass()
    res.sums, res.mag = np.array(out), np.array(mag)
    res.labels = np.where(sel, np.where(active, new, L_in), 0).astype(np.uint8)
    top = np.sort(logt, axis=0)
    with np.errstate(invalid="ignore"):
        res.gap = np.where(sel, top[-1] - top[-2], np.inf)
    res.scale = np.where(sel, np.abs(np.where(np.isfinite(logt), logt, 0.0)).max(axis=0), 0.0)
    res.selected = sel
    return res


def near_ties(res):
    """The selected voxels whose two best logt lie within 2^-30 max_k |logt_k| of each other: where a device label may differ."""
    return res.selected & (res.gap <= 2.0 ** -30 * res.scale)


def bound(n, mag, beta):
    """Per entry of the table, the family's bound (tissue_cases.bound: two float64 summations of n terms in different orders, and
    a few ulp on an exp argument of at most 745 with a 4x margin, 4 * 745 * 2^-52 < 2^-40) with the prior's roundings counted the
    same way: beta n_k (at most 6 * 8 = 48) is rounded once and its addition to a logt of magnitude up to 745 + 48 once more, each half an
    ulp of its result, 4 * (48 + 793) * 2^-53 < 2^-41 on the same exp argument.  Entry [1] also takes the normaliser: its terms
    count with their absolute values in `mag`, and exp(beta n_k) carries the rounding of its argument, 48 * 2^-53 relative, into
    log's result as an absolute error, 4 * 6 beta * 2^-53 per voxel with the same margin."""
    lim = (n * 2.0 ** -52 + 2.0 ** -40 + 2.0 ** -41) * np.asarray(mag, dtype=np.float64)
    lim[1] += n * 4.0 * 6.0 * min(float(beta), BETA_MAX) * 2.0 ** -53
    return lim


def label_table(params, classes, mistake=None):
    """lut[0] = 0, lut[1 + k] = 1 + the rank of class k by ascending mean (stable)."""
    mu = np.asarray(params)[classes:2 * classes]
    lut = np.zeros(classes + 1, dtype=np.uint8)
    if mistake == "labels_unsorted":
        lut[1:] = 1 + np.arange(classes)
    else:
        lut[1 + np.argsort(mu, kind="stable")] = 1 + np.arange(classes)
    return lut


def segment(x, mask=None, classes=3, order=3, iterations=60, beta=0.0, warmup=20, mistake=None, hook=None):
    """tissue_ref.segment with the prior: plain passes while t < warmup, the start pass (mode 2) at t == warmup, then mode t & 1 on
    two label buffers; after the last M-step two closing half-sweeps (modes 0, 1) with the final parameters; the labels are the
    prior's, renumbered by ascending mean.  beta == 0 is tissue_ref.segment, whatever the warm-up.  hook(kind) is called per pass with 'em', 0, 1 or 2."""
    K = classes
    hook = hook or (lambda kind: None)
    if beta > 0 and not 0 <= warmup < iterations:
        raise ValueError("tissue: warmup %d outside 0..%d" % (warmup, iterations - 1))
    if beta == 0:
        for _ in range(iterations):
            hook("em")
        return R.segment(x, mask, K, order, iterations, mistake=mistake)
    x = np.asarray(x)
    sel = R.selected(x, mask)
    n = int(sel.sum())
    if n < 100 * R.ncoef(order):
        raise ValueError("tissue: %d selected voxels, fewer than 100 per field term (%d)" % (n, 100 * R.ncoef(order)))
    params, v_floor = R.initial(np.log(x[sel].astype(np.float64)), K, order)
    res = R.Result()
    res.log_likelihood, res.trace = [], []
    L = None
    for t in range(iterations):
        if t < warmup:
            hook("em")
            sums = R.em_sums(x, mask, K, order, params)[0]
        else:
            mode = 2 if t == warmup else t & 1
            hook(mode)
            one = mrf_pass(x, mask, K, order, params, beta, mode, L, mistake)
            sums, L = one.sums, one.labels
        res.log_likelihood.append(float(sums[1]))
        res.trace.append(params)
        params = R.update(params, sums, K, order, v_floor)
    for mode in (0, 1):
        hook(mode)
        L = mrf_pass(x, mask, K, order, params, beta, mode, L, mistake).labels
    res.raw_labels, res.raw_params = L, params
    lut = label_table(params, K, mistake)
    params = R.sort_classes(R.finish(params, R._moments(sel.astype(np.float64), x.shape, order), n, K, order), K)
    res.params = params
    res.priors, res.means, res.variances, res.coefficients = R.split(params, K)
    res.restored, _plain_labels, res.field, res.gap = R.apply(x, mask, K, order, params)
    res.labels = lut[L]
    res.selected = n
    return res


def isolated(labels, mask):
    """Selected voxels none of whose six neighbours shares their label."""
    L = np.asarray(labels)
    n = neighbour_counts(L, int(L.max()) if L.max() > 0 else 1)
    own = np.zeros(L.shape, dtype=np.int64)
    for k in range(n.shape[0]):
        own += np.where(L == k + 1, n[k], 0)
    return int(((own == 0) & (np.asarray(mask) != 0) & (L > 0)).sum())


def figures(res, truth, P, mask):
    """(label agreement, field rms error, isolated voxels) against the phantom's truth."""
    rms, agree, _cv = R.end_to_end(res.restored, res.labels, res.field, truth, P, mask)
    return agree, rms, isolated(res.labels, mask)
