"""Parity cases of mri3d_tissue_mrf_pass (tests/test_tissue_mrf_gpu.py; tests/test_tissue_mrf_ref.py checks their near-ties and what
they cover).  The volumes are those of tests/tissue_cases.py, which reach every corner of the plan the two passes share, plus one
with D = 1 and one with H = 1, where no neighbour exists along that axis (order 0: tissue_cases says why).

A case runs at the parameters after 0 and after 5 reference iterations of the plain mixture; at each, the start pass (mode 2) once
and both colours at beta 0, 0.5 and 2.  labels_in of a colour pass is the start pass's label volume with bytes of 0 and of 200
scattered over 3 % of the voxels each, selected or not: neither counts for a class."""
import functools

import numpy as np

import tissue_cases as TC
import tissue_mrf_ref as M
import tissue_ref as R

# name: (shape, classes, order, mask kind); the names of tissue_cases.CASES take their volumes from there
EXTRA = {
    "d1_no_depth_neighbour": ((1, 9, 40), 3, 0, "blob"),
    "h1_no_height_neighbour": ((7, 1, 37), 4, 0, None),
}
CASES = dict(TC.CASES, **EXTRA)
ITERATIONS = (0, 5)
BETAS = (0.0, 0.5, 2.0)


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name in TC.CASES:
        return TC.inputs(name)
    shape, _K, _order, kind = CASES[name]
    x, s = TC.volume(shape, 20 + sorted(EXTRA).index(name))
    return x, ((s > np.quantile(s, 0.15)).astype(np.uint8) if kind == "blob" else None)


@functools.lru_cache(maxsize=None)
def parameters(name):
    """{iteration: params} of the plain mixture's reference loop."""
    shape, K, order, kind = CASES[name]
    if name in TC.CASES:
        return {it: ref[0] for it, ref in TC.reference(name).items() if it in ITERATIONS}
    x, mask = inputs(name)
    params, v_floor = R.initial(np.log(x[R.selected(x, mask)].astype(np.float64)), K, order)
    out = {}
    for it in range(max(ITERATIONS) + 1):
        if it in ITERATIONS:
            out[it] = params
        params = R.update(params, R.em_sums(x, mask, K, order, params)[0], K, order, v_floor)
    return out


def scattered(labels, seed):
    L = labels.copy().reshape(-1)
    rng = np.random.default_rng(seed)
    L[rng.random(L.size) < 0.03] = 0
    L[rng.random(L.size) < 0.03] = 200
    return L.reshape(labels.shape)


@functools.lru_cache(maxsize=None)
def reference(name):
    """[(iteration, beta, mode, params, labels_in or None, the reference's Pass)], computed once and left unchanged."""
    shape, K, order, _kind = CASES[name]
    x, mask = inputs(name)
    out = []
    for it, params in sorted(parameters(name).items()):
        start = M.mrf_pass(x, mask, K, order, params, 0.5, 2, None)
        out.append((it, 0.5, 2, params, None, start))
        L = scattered(start.labels, 7 + it)
        for beta in BETAS:
            for mode in (0, 1):
                out.append((it, beta, mode, params, L, M.mrf_pass(x, mask, K, order, params, beta, mode, L)))
    return out
