"""The outputs of the tissue family whose bits tests/golden/tissue_family_bits.json records (tools/record_tissue_bits.py writes the
file, tests/test_tissue_mrf_gpu.py recomputes every entry).  Every entry is the sha256 of one output's bytes.

The parity inputs: `em_pass` on every case of tests/tissue_cases.py at each of its iterations; `apply` on the same cases at the last
of them with the classes in reverse order, out of place with the field and in place without; `mrf_pass` on every entry of
tissue_mrf_cases.reference(name).  Those reach 6 of the 12 (classes, order) instances of the row kernels, so a sweep runs all 12 on
the volume of "w37_odd_rows" at parameters from a formula (no M-step is run: any order goes with any shape): `em_pass`, `mrf_pass`
in mode 2 and in modes 0 and 1 at beta 0.5 on the start pass's labels, scattered, and `apply` once per class count."""
import hashlib

import numpy as np
import torch

import tissue_cases as TC
import tissue_mrf_cases as MC
import tissue_ref as R

SWEEP_VOLUME, SWEEP_BETA = "w37_odd_rows", 0.5


def sweep_params(K, order):
    """pi_k ~ k + 1, means evenly over log 0.3 .. log 1, v_k = 0.02 + 0.01 k, c_n = 0.15 sin(1 + 2 n)."""
    k = np.arange(K, dtype=np.float64)
    pi = (k + 1.0) / (k + 1.0).sum()
    mu = np.log(0.3) + (np.log(1.0) - np.log(0.3)) * k / (K - 1)
    return np.concatenate([pi, mu, 0.02 + 0.01 * k, 0.15 * np.sin(1.0 + 2.0 * np.arange(R.ncoef(order)))])


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _apply_bits(ops, out, key, dx, dm, K, order, params):
    rest, lab, fld = ops.tissue_apply(dx, dm, K, order, params, want_field=True)
    out[key + "/restored"], out[key + "/labels"], out[key + "/field"] = _sha(rest), _sha(lab), _sha(fld)
    x2 = dx.clone()
    rest, lab, _none = ops.tissue_apply(x2, dm, K, order, params, restored=x2)
    out[key + "/in_place/restored"], out[key + "/in_place/labels"] = _sha(rest), _sha(lab)


def device_bits(ops):
    """{entry: sha256} of every recorded output, computed on the device."""
    out = {}
    for name in sorted(TC.CASES):
        _shape, K, order, _kind = TC.CASES[name]
        dx, dm = (_dev(a) for a in TC.inputs(name))
        ref = TC.reference(name)
        for it, (params, _sums, _mag) in sorted(ref.items()):
            out["em_pass/%s/it%d" % (name, it)] = _sha(ops.tissue_em_pass(dx, dm, K, order, params))
        pi, mu, v, c = R.split(ref[max(ref)][0], K)
        _apply_bits(ops, out, "apply/%s" % name, dx, dm, K, order, np.concatenate([pi[::-1], mu[::-1], v[::-1], c]))
    for name in sorted(MC.CASES):
        _shape, K, order, _kind = MC.CASES[name]
        dx, dm = (_dev(a) for a in MC.inputs(name))
        for it, beta, mode, params, labels_in, _want in MC.reference(name):
            sums, lab = ops.tissue_mrf_pass(dx, dm, K, order, params, beta, mode, _dev(labels_in))
            key = "mrf_pass/%s/it%d-beta%g-mode%d" % (name, it, beta, mode)
            out[key + "/sums"], out[key + "/labels"] = _sha(sums), _sha(lab)
    dx, dm = (_dev(a) for a in TC.inputs(SWEEP_VOLUME))
    for K in (2, 3, 4):
        for order in (0, 1, 2, 3):
            params, key = sweep_params(K, order), "sweep/K%d-order%d" % (K, order)
            out[key + "/em_pass"] = _sha(ops.tissue_em_pass(dx, dm, K, order, params))
            sums, start = ops.tissue_mrf_pass(dx, dm, K, order, params, SWEEP_BETA, 2, None)
            out[key + "/mrf_start/sums"], out[key + "/mrf_start/labels"] = _sha(sums), _sha(start)
            scattered = _dev(MC.scattered(start.cpu().numpy(), 7))
            for mode in (0, 1):
                sums, lab = ops.tissue_mrf_pass(dx, dm, K, order, params, SWEEP_BETA, mode, scattered)
                out[key + "/mrf_colour%d/sums" % mode], out[key + "/mrf_colour%d/labels" % mode] = _sha(sums), _sha(lab)
        _apply_bits(ops, out, "sweep/K%d/apply" % K, dx, dm, K, 3, sweep_params(K, 3))
    return out
