"""The tissue family's five calls from two builds of the library, alternated in one process on one MI355X.  Not collected by pytest.

    python tests/perf/tissue_family_ab.py --other OTHER_LIBRARY.so [--rounds 2] [--out profiles/tissue_family_walk.txt]

For a change of csrc/tissue.hip that means to keep bits and speed: OTHER_LIBRARY.so is libmri3d_hip.so built from the commit before
it.  Workload and method are tests/perf/tissue_mrf_bench.py's: the phantom of tests/tissue_mrf_ref.py at noise 0.10 on the template's
grid 182x218x182, head mask, classes 3, order 3, the parameters after two EM iterations; device events around 20 back-to-back calls
after a warm-up window, three windows.  `em_pass`, `mrf_pass` (the start pass and both colours, beta 1) and `apply` (with the field)
are timed; a round runs every call from the other library and then from this tree's, and every window is printed.  Before the first
round each call's outputs from the two libraries are compared byte for byte.  There is no bar here: the margin is the other
library's own window-to-window spread in the same session."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tissue_bench import windows  # noqa: E402

SHAPE, K, ORDER, BETA, NOISE = (182, 218, 182), 3, 3, 1.0, 0.10
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def main():
    import numpy as np
    import torch

    import tissue_mrf_ref as M
    from mri_epilepsy_diagnosis_amd import _lib, ops, tissue

    other = ctypes.CDLL(sys.argv[sys.argv.index("--other") + 1])
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith("mri3d_tissue"):
            getattr(other, name).restype, getattr(other, name).argtypes = res, args
    libs = (("other", other), ("this ", _lib.lib()))
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 2
    P, st = ops._ptr, ops._stream()
    say("device %s; %dx%dx%d, classes %d, order %d, beta %g, phantom noise %g" % ((torch.cuda.get_device_name(0),) + SHAPE + (K, ORDER, BETA, NOISE)))
    x, mask, _truth, _field, _img = M.phantom(0, NOISE, SHAPE)
    dx, dm = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
    warm = tissue.segment(dx, dm, classes=K, order=ORDER, iterations=2)
    params = np.ascontiguousarray(np.concatenate([warm.priors, warm.means, warm.variances, warm.coefficients]))
    hp = params.ctypes.data_as(ctypes.c_void_p)
    ws = ops._workspace(_lib.lib().mri3d_tissue_em_workspace_bytes(*SHAPE, K, ORDER), dx.device)
    sums = torch.empty(ops.tissue_table_size(K, ORDER), dtype=torch.float64, device="cuda")
    lin, lout, lab = (torch.empty(SHAPE, dtype=torch.uint8, device="cuda") for _ in range(3))
    rest, fld = torch.empty_like(dx), torch.empty_like(dx)
    assert other.mri3d_tissue_mrf_pass(P(dx), P(dm), *SHAPE, K, ORDER, hp, BETA, 2, None, P(lin), P(sums), P(ws), ws.numel(), st) == 0

    def calls(L):
        out = [("em_pass          ", lambda: L.mri3d_tissue_em_pass(P(dx), P(dm), *SHAPE, K, ORDER, hp, P(sums), P(ws), ws.numel(), st), (sums,))]
        for mode, name in ((2, "mrf_pass start   "), (0, "mrf_pass colour 0"), (1, "mrf_pass colour 1")):
            out.append((name, lambda mode=mode: L.mri3d_tissue_mrf_pass(P(dx), P(dm), *SHAPE, K, ORDER, hp, BETA, mode, P(lin) if mode != 2 else None,
                                                                        P(lout), P(sums), P(ws), ws.numel(), st), (sums, lout)))
        out.append(("apply            ", lambda: L.mri3d_tissue_apply(P(dx), P(dm), *SHAPE, K, ORDER, hp, P(rest), P(lab), P(fld), st), (rest, lab, fld)))
        return out

    results = []
    for _tag, L in libs:
        got = []
        for _name, call, outs in calls(L):
            for t in outs:
                t.view(torch.uint8).fill_(0xA5)
            assert call() == 0
            torch.cuda.synchronize()
            got.append([t.clone() for t in outs])
        results.append(got)
    for (name, _call, _outs), a, b in zip(calls(other), *results):
        assert all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(a, b)), name
    say("every output of the five calls: the same bytes from both libraries")
    for r in range(rounds):
        for tag, L in libs:
            for name, call, _outs in calls(L):
                w = windows(call, 20)
                say("RESULT round %d %s %s  %.4f ms  (windows %s)" % (r, tag, name, min(w), " ".join("%.4f" % v for v in w)))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
