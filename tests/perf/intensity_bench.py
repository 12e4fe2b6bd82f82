"""The intensity statistics (csrc/intensity.hip) on one MI355X.  Not collected by pytest.

    python tests/perf/intensity_bench.py [--out profiles/intensity_bench.txt] [--no-cpu]

Workload: one T1-like 160x192x160 volume and a stack of 4, m = 100 positions, Scott's rule.  Moments and KDE are timed apart: device
events around n back-to-back calls after a warm-up window, three windows, the best one reported (the spread beside it).  A pair is
one (voxel, position) exponential: voxels x 100 per volume; pairs per second are set against the estimate DESIGN 4.12 derives from
the issue costs of the instructions.  train_landmarks over 8 volumes is wall clock (it crosses to the host once per volume).
The CPU side is one scipy.stats.gaussian_kde run over the same volume on this machine's CPU, or tests/intensity_ref.py where scipy is
missing; the line says which, and how far the device result is from it.  There is no bar: the path is new."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VOL, M = (160, 192, 160), 100
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
    import numpy as np
    import torch
    import intensity_ref
    from mri_epilepsy_diagnosis_amd import _lib, ops
    from mri_epilepsy_diagnosis_amd.classification import preprocessing

    L, P, st = _lib.lib(), ops._ptr, ops._stream()
    nvox = VOL[0] * VOL[1] * VOL[2]
    host = np.stack([intensity_ref.t1_like(300 + k, (nvox,)) * np.float32(1 + k) for k in range(4)])
    stack = torch.from_numpy(host).cuda()
    plan = (torch.zeros(4, dtype=torch.int32)).numpy()
    assert L.mri3d_kde_plan(nvox, 1, M, plan.ctypes.data) == 0
    say("device %s; volume %dx%dx%d = %d voxels, m = %d; plan: %d blocks per volume, %d voxels per tile, %d slots per lane, %d trips"
        % ((torch.cuda.get_device_name(0),) + VOL + (nvox, M) + tuple(int(v) for v in plan)))
    for batch in (1, 4):
        x = stack[:batch]
        mom = torch.empty((batch, 8), dtype=torch.float64, device="cuda")
        pos = torch.empty((batch, M), dtype=torch.float64, device="cuda")
        den = torch.empty((batch, M), dtype=torch.float64, device="cuda")
        ws = ops._workspace(L.mri3d_intensity_workspace_bytes(nvox, batch, M), x.device)
        f_mom = lambda: L.mri3d_intensity_moments_f32(P(x), None, nvox, batch, P(mom), P(ws), ws.numel(), st)   # noqa: E731
        f_kde = lambda: L.mri3d_kde_f32(P(x), None, nvox, batch, P(mom), None, M, 0, 0.0, P(pos), P(den), P(ws), ws.numel(), st)   # noqa: E731
        w = windows(f_mom, 50)
        say("RESULT moments  batch %d   %.4f ms  (windows %s)  %.3f TB/s" % (batch, min(w), " ".join("%.4f" % v for v in w),
                                                                           4.0 * nvox * batch / min(w) / 1e9))
        w = windows(f_kde, 20)
        pairs = float(nvox) * M * batch
        say("RESULT kde      batch %d   %.4f ms  (windows %s)  %.3e pairs/s  (%.4f ms per volume)"
            % (batch, min(w), " ".join("%.4f" % v for v in w), pairs / (min(w) * 1e-3), min(w) / batch))
    device_density = den[0].cpu().numpy()
    device_positions = pos[0].cpu().numpy()

    vols = [stack[k % 4].view(VOL) * (1.0 + 0.1 * (k // 4)) for k in range(8)]
    preprocessing.train_landmarks(vols[:1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    landmarks = preprocessing.train_landmarks(vols)
    torch.cuda.synchronize()
    say("RESULT train_landmarks over 8 volumes   %.1f ms wall  (landmarks %.3f .. %.3f)" % ((time.perf_counter() - t0) * 1e3, landmarks[0], landmarks[-1]))

    if "--no-cpu" not in sys.argv:
        try:
            from scipy.stats import gaussian_kde
            t0 = time.perf_counter()
            want = gaussian_kde(host[0])(device_positions)
            who = "scipy %s gaussian_kde" % __import__("scipy").__version__
        except ImportError:
            t0 = time.perf_counter()
            _, want = intensity_ref.kde_ref(host[0], positions=device_positions)
            who = "tests/intensity_ref.py kde_ref (scipy is not installed here)"
        say("RESULT cpu: %s over the same volume   %.2f s on this machine's CPU; device density off by %.3e of its maximum"
            % (who, time.perf_counter() - t0, np.abs(device_density - want).max() / want.max()))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
