"""The two kernels of the Monte-Carlo predictive statistics (csrc/mc_stats.hip) against `mri3d_add_channels` on one MI355X, and the
cost of `mc_predict` on the variational-dropout U-Net.  Not collected by pytest.

    python tests/perf/mc_bench.py                 # every measurement, each in a child process under its own time limit
    python tests/perf/mc_bench.py --only NAME     # one measurement in this process (what the children run)

Kernels: N = 4 volumes of 160x192x160 with C = 2 classes (dense NDHWC logits, fp32 and bf16), device events around `n`
back-to-back calls after a warm-up window, best of three windows.  The state (5 floats per voxel = 393 MB) plus the logits exceed
the 256 MiB Infinity Cache, so the figures are HBM figures.  Bytes are the algorithmic traffic per voxel:
  accumulate   reps x C logits read once; the state (2C + 1 floats) read and written once per call (written only when first = 1)
  finalize     the state read once; mean, variance (C floats each), entropy, mutual_info (1 float each) and the mask (1 byte) written
Yardstick in the same run: mri3d_add_channels at 16 channels on one 160x192x160 volume.  The bar of the feature: each new kernel at
>= 0.8x the bytes/s of add_channels (fp32) in the same run.
Model: UNet3D(2, bayes=True) at its default widths on 1x1x160x192x160, mc_predict(n_samples=8), and the share of that time the two
new kernels take (their own timings at N = 1 in the same process: 8 accumulate calls + 1 finalize).
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, C, VOL = 4, 2, (160, 192, 160)
KERNELS = ["add_channels", "mc_accumulate_first", "mc_accumulate", "mc_accumulate_reps4", "mc_finalize"]
LIMITS = {"model": 420}      # seconds per child; kernels: 120


def timed(fn, n, repeats=3):
    import torch
    best = float("inf")
    for r in range(repeats + 1):          # window 0 is the warm-up
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        if r:
            best = min(best, start.elapsed_time(stop) / n)
    return best


def _report(name, kind, ms, nbytes, per_vox):
    print("RESULT %-20s %-4s %.4f ms  %.3f TB/s  (%s B/voxel)" % (name, kind, ms, nbytes / ms / 1e9, per_vox), flush=True)


def bench_kernel(name):
    import torch
    from mri_epilepsy_diagnosis_amd import _lib, ops
    L = _lib.lib()
    P, st = ops._ptr, ops._stream()
    vol = VOL[0] * VOL[1] * VOL[2]
    if name == "add_channels":
        for dtype, dt, esz in ((torch.float32, _lib.F32, 4), (torch.bfloat16, _lib.BF16, 2)):
            a, b = (torch.randn(vol, 16, device="cuda").to(dtype) for _ in range(2))
            out = torch.empty_like(a)
            fn = lambda: L.mri3d_add_channels(P(a), P(b), P(out), vol, 16, 16, 16, 16, dt, st)   # noqa: E731
            assert fn() == 0, L.mri3d_last_error()
            _report(name, "bf16" if esz == 2 else "fp32", timed(fn, 300), 3 * esz * vol * 16, 3 * esz * 16)
        return
    nvox = N * vol
    sbytes = L.mri3d_mc_state_bytes(nvox, C)
    state = torch.zeros(sbytes // 4, device="cuda")
    sfl = 2 * C + 1
    for dtype, dt, esz in ((torch.float32, _lib.F32, 4), (torch.bfloat16, _lib.BF16, 2)):
        kind = "bf16" if esz == 2 else "fp32"
        if name.startswith("mc_accumulate"):
            reps = 4 if name.endswith("reps4") else 1
            first = 1 if name.endswith("first") else 0
            logits = (3.0 * torch.randn(reps * nvox, C, device="cuda")).to(dtype)
            fn = lambda: L.mri3d_mc_accumulate(P(logits), nvox, C, C, dt, reps, nvox, first, P(state), sbytes, st)   # noqa: E731
            per = reps * C * esz + (1 if first else 2) * 4 * sfl
            n = 100
        else:
            if esz == 2:
                return                        # finalize has no storage type: the state and its outputs are fp32
            kind = "fp32"
            logits = (3.0 * torch.randn(nvox, C, device="cuda"))
            assert L.mri3d_mc_accumulate(P(logits), nvox, C, C, dt, 1, nvox, 1, P(state), sbytes, st) == 0, L.mri3d_last_error()
            del logits
            mean, var = torch.empty(nvox, C, device="cuda"), torch.empty(nvox, C, device="cuda")
            ent, mi = torch.empty(nvox, device="cuda"), torch.empty(nvox, device="cuda")
            mask = torch.empty(nvox, dtype=torch.uint8, device="cuda")
            fn = lambda: L.mri3d_mc_finalize(P(state), sbytes, nvox, C, 1, P(mean), P(var), P(ent), P(mi), P(mask), st)   # noqa: E731
            per = 4 * sfl + 4 * (2 * C + 2) + 1
            n = 100
        assert fn() == 0, L.mri3d_last_error()
        _report(name, kind, timed(fn, n), per * nvox, per)
        if name.startswith("mc_accumulate"):
            del logits
            torch.cuda.empty_cache()


def bench_model():
    import torch
    from mri_epilepsy_diagnosis_amd import ops
    from mri_epilepsy_diagnosis_amd.segmentation.models.bayes_unet import UNet3D
    from mri_epilepsy_diagnosis_amd.segmentation.uncertainty import mc_predict
    x = torch.randn(1, 1, *VOL, generator=torch.Generator().manual_seed(0)).cuda()
    torch.manual_seed(0)
    m = UNet3D(2, bayes=True).cuda()
    samples = 8
    ms = timed(lambda: mc_predict(m, x, n_samples=samples), 2, repeats=2)
    with torch.no_grad():
        m.eval()
        logits = m(x)
    del m
    torch.cuda.empty_cache()
    state = ops.mc_state(logits.shape, logits.device)
    ops.mc_accumulate(state, logits, True)
    acc = timed(lambda: ops.mc_accumulate(state, logits, False), 50)
    fin = timed(lambda: ops.mc_finalize(state, logits.shape, samples), 50)
    own = samples * acc + fin
    print("RESULT mc_predict(n_samples=%d) UNet3D(2, bayes=True) 1x1x160x192x160 fp32: %.1f ms; accumulate %.4f ms per draw, "
          "finalize %.4f ms (with its output allocations): %.3f ms = %.2f %% of the call"
          % (samples, ms, acc, fin, own, 100.0 * own / ms), flush=True)


if __name__ == "__main__":
    if "--only" in sys.argv:
        what = sys.argv[sys.argv.index("--only") + 1]
        bench_model() if what == "model" else bench_kernel(what)
        sys.exit(0)
    for what in KERNELS + ["model"]:      # one child at a time; after a child that failed or ran out of time nothing more is started
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", what], timeout=LIMITS.get(what, 120),
                               capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            sys.exit("mc_bench: %s ran past its time limit; stopping" % what)
        sys.stdout.write("".join(line + "\n" for line in r.stdout.splitlines() if line.startswith("RESULT")))
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            sys.exit("mc_bench: %s ended with status %d; stopping" % (what, r.returncode))
