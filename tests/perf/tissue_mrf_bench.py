"""The tissue classes' pass with the Potts prior (mri3d_tissue_mrf_pass) against the plain pass on one MI355X.  Not
collected by pytest.

    python tests/perf/tissue_mrf_bench.py [--out profiles/tissue_mrf_bench.txt]

Workload and method are tests/perf/tissue_bench.py's: the phantom of tests/tissue_mrf_ref.py at noise 0.10 on the template's grid
182x218x182 and on 160x192x160, head mask, classes 3, order 3, the parameters after two EM iterations; device events around 20
back-to-back calls after a warm-up window, three windows, the best one reported (all three beside it).  `em_pass` and `mrf_pass`
(the start pass and both colours, beta 1, labels_in the start pass's output) are timed on the same volumes in the same run.
The row kernels' shares come from one torch-profiler window of ten calls.  `segment` (60 iterations, warmup 20) with beta 0 and
with beta 1 is wall clock around a device synchronise, run twice, the second reported, with its end-to-end figures.  There is no
bar: the path is new."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tissue_bench import windows  # noqa: E402

SHAPES, K, ORDER, BETA, NOISE = ((182, 218, 182), (160, 192, 160)), 3, 3, 1.0, 0.10
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def main():
    import ctypes

    import numpy as np
    import torch
    from torch.profiler import ProfilerActivity, profile

    import tissue_mrf_ref as M
    from mri_epilepsy_diagnosis_amd import _lib, ops, tissue

    L, P, st = _lib.lib(), ops._ptr, ops._stream()
    say("device %s; classes %d, order %d, beta %g, phantom noise %g" % (torch.cuda.get_device_name(0), K, ORDER, BETA, NOISE))
    for shape in SHAPES:
        x, mask, truth, Pfield, _img = M.phantom(0, NOISE, shape)
        dx, dm = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
        tag = "%dx%dx%d" % shape
        warm = tissue.segment(dx, dm, classes=K, order=ORDER, iterations=2)
        params = np.ascontiguousarray(np.concatenate([warm.priors, warm.means, warm.variances, warm.coefficients]))
        hp = params.ctypes.data_as(ctypes.c_void_p)
        plan = ops.tissue_em_plan(shape, K, ORDER)
        ws = ops._workspace(L.mri3d_tissue_em_workspace_bytes(*shape, K, ORDER), dx.device)
        sums = torch.empty(plan["entries"], dtype=torch.float64, device="cuda")
        lin, lout = (torch.empty(shape, dtype=torch.uint8, device="cuda") for _ in range(2))
        assert L.mri3d_tissue_mrf_pass(P(dx), P(dm), *shape, K, ORDER, hp, BETA, 2, None, P(lin), P(sums), P(ws), ws.numel(), st) == 0
        calls = [("em_pass          ", lambda: L.mri3d_tissue_em_pass(P(dx), P(dm), *shape, K, ORDER, hp, P(sums), P(ws), ws.numel(), st))]
        for mode, name in ((2, "mrf_pass start   "), (0, "mrf_pass colour 0"), (1, "mrf_pass colour 1")):
            calls.append((name, lambda mode=mode: L.mri3d_tissue_mrf_pass(P(dx), P(dm), *shape, K, ORDER, hp, BETA, mode, P(lin) if mode != 2 else None,
                                                                          P(lout), P(sums), P(ws), ws.numel(), st)))
        base = None
        for name, call in calls:
            w = windows(call, 20)
            ms = min(w)
            base = base or ms
            say("RESULT %s %s head mask   %.4f ms  (windows %s)  %.2f x em_pass" % (name, tag, ms, " ".join("%.4f" % v for v in w), ms / base))
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                assert calls[0][1]() == 0 and calls[2][1]() == 0
            torch.cuda.synchronize()
        for e in prof.key_averages():
            if "tissue_" in e.key:
                say("RESULT %s kernel %-40s %.4f ms a call" % (tag, e.key.split("(")[0][:40], getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / e.count / 1e3))
        for beta in (0.0, BETA):
            for attempt in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = tissue.segment(dx, dm, classes=K, order=ORDER, iterations=60, beta=beta, warmup=20)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0

            class Host:
                restored, labels, field = res.restored.cpu().numpy(), res.labels.cpu().numpy(), res.field.cpu().numpy()
            agree, rms, isolated = M.figures(Host, truth, Pfield, mask)
            say("RESULT segment %s 60 iterations, beta %g   %.3f s wall  (%d selected voxels; label agreement %.4f, field rms error %.4f, "
                "isolated voxels %d)" % (tag, beta, wall, res.selected, agree, rms, isolated))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
