"""The streaming kernels of BayesConv3d (csrc/bayes.hip) against `mri3d_add_channels` on one MI355X, and the cost of a
variational-dropout U-Net step against the plain one.  Not collected by pytest.

    python tests/perf/bayes_bench.py                 # every measurement, each in a child process under its own time limit
    python tests/perf/bayes_bench.py --only NAME     # one measurement in this process (what the children run)

Kernels: 16 channels at 160x192x160 (dense NDHWC), fp32 and bf16, device events around `n` back-to-back calls after a warm-up
window, best of three windows.  Bytes are the algorithmic traffic: every input read once, every output written once (eps is
always fp32).  The bar of the feature: each new kernel at >= 0.8x the bytes/s of add_channels in the same run.
Model: UNet3D(2) at its default widths [1, 16, 32, 64, 128] on 1x1x160x192x160, forward + softmax-Dice + backward, eager.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

C, VOL = 16, (160, 192, 160)
KERNELS = ["add_channels", "bayes_square", "bayes_sample_fwd", "bayes_sample_bwd", "bayes_dx"]
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


def bench_kernel(name):
    import torch
    from mri_epilepsy_diagnosis_amd import _lib, ops
    L = _lib.lib()
    nvox = VOL[0] * VOL[1] * VOL[2]
    eps = torch.randn(nvox, C, device="cuda")
    for dtype, dt, esz in ((torch.float32, _lib.F32, 4), (torch.bfloat16, _lib.BF16, 2)):
        a, b, c = (torch.randn(nvox, C, device="cuda").abs().to(dtype) for _ in range(3))
        out = torch.empty_like(a)
        P, st = ops._ptr, ops._stream()
        calls = {
            "add_channels": (3 * esz, lambda: L.mri3d_add_channels(P(a), P(b), P(out), nvox, C, C, C, C, dt, st)),
            "bayes_square": (2 * esz, lambda: L.mri3d_bayes_square(P(a), P(out), nvox, C, C, C, dt, st)),
            "bayes_sample_fwd": (3 * esz + 4, lambda: L.mri3d_bayes_sample_fwd(P(a), P(b), P(eps), P(out), nvox, C, C, C, C, C, dt, st)),
            "bayes_sample_bwd": (3 * esz + 4, lambda: L.mri3d_bayes_sample_bwd(P(a), P(b), P(eps), P(out), nvox, C, C, C, C, C, dt, st)),
            "bayes_dx": (4 * esz, lambda: L.mri3d_bayes_dx(P(a), P(b), P(c), P(out), nvox, C, C, C, C, C, dt, st)),
        }
        per_elem, fn = calls[name]
        assert fn() == 0, L.mri3d_last_error()
        ms = timed(fn, 300)
        nbytes = per_elem * nvox * C
        print("RESULT %-17s %-4s %.4f ms  %.3f TB/s  (%d B/element)" % (name, "bf16" if esz == 2 else "fp32", ms, nbytes / ms / 1e9, per_elem),
              flush=True)


def bench_model():
    import torch
    from mri_epilepsy_diagnosis_amd import ops
    from mri_epilepsy_diagnosis_amd.segmentation.models.bayes_unet import UNet3D
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 1, *VOL, generator=g).cuda()
    t = (torch.rand(1, 1, *VOL, generator=g) < 0.1).float().cuda()
    for bayes in (False, True):
        torch.manual_seed(0)
        m = UNet3D(2, bayes=bayes).cuda().train()

        def step():
            m.zero_grad(set_to_none=True)
            ops.softmax_dice_loss(m(x), t).backward()
        ms = timed(step, 4, repeats=2)
        print("RESULT UNet3D(2, bayes=%s) 1x1x160x192x160 fp32: %.1f ms per forward+backward step, peak memory %.1f GB"
              % (bayes, ms, torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
        del m
        torch.cuda.empty_cache()


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
            sys.exit("bayes_bench: %s ran past its time limit; stopping" % what)
        sys.stdout.write("".join(line + "\n" for line in r.stdout.splitlines() if line.startswith("RESULT")))
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            sys.exit("bayes_bench: %s ended with status %d; stopping" % (what, r.returncode))
