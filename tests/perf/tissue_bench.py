"""Bias-field estimation over tissue classes (csrc/tissue.hip, mri_epilepsy_diagnosis_amd/tissue) on one MI355X.  Not collected by
pytest.

    python tests/perf/tissue_bench.py [--out profiles/tissue_bench.txt] [--no-cpu]

Workload: the phantom of tests/tissue_ref.py (three tissues, a cubic bias field, a spherical head mask) on the template's grid
182x218x182 and on 160x192x160; classes 3, order 3, the parameters after two EM iterations.  `em_pass` and `apply` are timed with
device events around n back-to-back calls after a warm-up window, three windows, the best one reported (all three beside it).
Algorithmic bytes of a pass: x (4 B) and the mask (1 B) per voxel, the per-row sums written once and read by every table entry
that folds them; TB/s is that over the call time, an end-to-end figure of the two launches.  The two kernels' shares come from
one torch-profiler window of ten calls (kernel tracing alone, no counters).  `segment` (60 iterations, one table to the host per
iteration) is wall clock around a device synchronise, run twice, the second reported.  The host restatement is one pass of
tests/tissue_ref.py (float64 numpy) on this machine's CPU.  There is no bar: the path is new."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES, K, ORDER = ((182, 218, 182), (160, 192, 160)), 3, 3
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def windows(fn, n, repeats=3):
    import torch
    out = []
    for r in range(repeats + 1):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            assert fn() == 0
        stop.record()
        stop.synchronize()
        if r:
            out.append(start.elapsed_time(stop) / n)
    return out


def main():
    import ctypes

    import numpy as np
    import torch
    from torch.profiler import ProfilerActivity, profile

    import tissue_ref as R
    from mri_epilepsy_diagnosis_amd import _lib, ops, tissue

    L, P, st = _lib.lib(), ops._ptr, ops._stream()
    say("device %s; classes %d, order %d" % (torch.cuda.get_device_name(0), K, ORDER))
    for shape in SHAPES:
        x, mask, truth, Pfield, _img = R.phantom(0, shape)
        dx, dm = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
        nvox, nsel = x.size, int((mask != 0).sum())
        tag = "%dx%dx%d" % shape
        # the parameters after two device iterations
        warm = tissue.segment(dx, dm, classes=K, order=ORDER, iterations=2)
        params = np.ascontiguousarray(np.concatenate([warm.priors, warm.means, warm.variances, warm.coefficients]))
        hp = params.ctypes.data_as(ctypes.c_void_p)
        plan = ops.tissue_em_plan(shape, K, ORDER)
        need = L.mri3d_tissue_em_workspace_bytes(*shape, K, ORDER)
        ws = ops._workspace(need, dx.device)
        sums = torch.empty(plan["entries"], dtype=torch.float64, device="cuda")
        for name, m in (("head mask", dm), ("no mask  ", None)):
            call = lambda: L.mri3d_tissue_em_pass(P(dx), P(m), *shape, K, ORDER, hp, P(sums), P(ws), ws.numel(), st)  # noqa: E731
            w = windows(call, 20)
            ms = min(w)
            counted = nsel if m is not None else nvox
            nbytes = nvox * (4 + (1 if m is not None else 0)) + plan["row_sums"] * plan["rows"] * 8 + 8 * plan["rows"] * plan["entries"]
            say("RESULT em_pass %s %s   %.4f ms  (windows %s)  %.3e selected voxels/s  %.3f TB/s algorithmic  (%d blocks, %d trips, "
                "%d wave steps a row, %d sums a row, %d table entries)"
                % (tag, name, ms, " ".join("%.4f" % v for v in w), counted / (ms * 1e-3), nbytes / ms / 1e9, plan["blocks"], plan["trips"],
                   plan["wave_steps"], plan["row_sums"], plan["entries"]))
        call = lambda: L.mri3d_tissue_em_pass(P(dx), P(dm), *shape, K, ORDER, hp, P(sums), P(ws), ws.numel(), st)  # noqa: E731
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                assert call() == 0
            torch.cuda.synchronize()
        for e in prof.key_averages():
            if "tissue_em" in e.key:
                say("RESULT em_pass %s head mask  kernel %-40s %.4f ms a call" % (tag, e.key.split("(")[0][:40], getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / e.count / 1e3))
        rest, lab, fld = torch.empty_like(dx), torch.empty(shape, dtype=torch.uint8, device="cuda"), torch.empty_like(dx)
        for name, f in (("with field", fld), ("no field  ", None)):
            call = lambda: L.mri3d_tissue_apply(P(dx), P(dm), *shape, K, ORDER, hp, P(rest), P(lab), P(f), st)  # noqa: E731
            w = windows(call, 20)
            ms = min(w)
            nbytes = nvox * (4 + 1 + 4 + 1 + (4 if f is not None else 0))
            say("RESULT apply   %s %s  %.4f ms  (windows %s)  %.3f TB/s algorithmic" % (tag, name, ms, " ".join("%.4f" % v for v in w), nbytes / ms / 1e9))
        for attempt in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tissue.segment(dx, dm, classes=K, order=ORDER, iterations=60)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        rms, agree, cv = R.end_to_end(res.restored.cpu().numpy(), res.labels.cpu().numpy(), res.field.cpu().numpy(), truth, Pfield, mask)
        say("RESULT segment %s 60 iterations   %.3f s wall  (%d selected voxels; field rms error %.4f, label agreement %.4f, CV over "
            "class 3 %.4f)" % (tag, wall, res.selected, rms, agree, cv))
        if "--no-cpu" not in sys.argv:
            t0 = time.perf_counter()
            want, mag = R.em_sums(x, mask, K, ORDER, params)
            cpu_s = time.perf_counter() - t0
            assert call() == 0
            got = sums.cpu().numpy()
            over = np.abs(got - want) / np.maximum((want[0] * 2.0 ** -52 + 2.0 ** -40) * mag, 1e-300)
            say("RESULT cpu: one pass of the float64 numpy restatement (both tables) %s   %.2f s on this machine's CPU; the device "
                "table is within %.3f of the counted bound" % (tag, cpu_s, over.max()))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
