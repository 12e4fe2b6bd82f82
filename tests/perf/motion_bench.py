"""The motion artefact (RandomMotion) on one MI355X: S = 2 volumes of 160x192x160 at K = 2 moved copies, timed with device
events after a warm-up pass (best of 3 averages over windows of 0.15 s and more).
  (a) `mri3d_kspace_mix_f32` alone: K + 1 volumes in, one out — algorithmic bytes (K + 2) 4 V, V = voxels of the batch;
  (b) the whole `Motion` step as `transforms.execute` runs it: the input copied into slot 0, the minimum of each image, K warps
      per subject, the mix;
  (c) the yardstick, the route the library definition implies, on the same device and fed the same moved copies:
      `torch.fft.fftn` of the K + 1 volumes, slab copy along the last axis, `ifftn`, `.real`.  The slabs are copied at their
      unshifted positions, which spares (c) the two fftshift passes.  If torch.fft is not usable here, that is said and
      (a) and (b) stand alone.
    python tests/perf/motion_bench.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mri_epilepsy_diagnosis_amd.segmentation import transforms as T  # noqa: E402


def timed(fn, n, repeats=3):
    """best of `repeats` averages over n calls (ms per call) between two device events, after a warm-up pass"""
    best = float("inf")
    for r in range(repeats + 1):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        if r:
            best = min(best, start.elapsed_time(stop) / n)
    return best


S, K, shape = 2, 2, (160, 192, 160)
W = shape[2]
nvox = S * int(np.prod(shape))
image = (torch.randn((S,) + shape, generator=torch.Generator().manual_seed(0)) * 30 + 5).cuda()
rng = np.random.default_rng(0)
motion = T.RandomMotion(num_transforms=K)
plans, slabs = [], []
for _ in range(S):
    plans.append(T.fold(motion.plan(shape, rng)[0]))
    slabs.append(motion.last_params["slabs"])
steps = [p[0] for p in plans]

# the moved copies, made once: (a) and (c) read the same buffer
buf = torch.empty((S, K + 1) + shape, dtype=torch.float32, device="cuda")
buf[:, 0].copy_(image)
pad = T._minimum(image)
for i, st in enumerate(steps):
    for k in range(K):
        T.warp3d(image[i:i + 1], None, st.matrices[k, :3][None], None, pad[i:i + 1], image_out=buf[i, k + 1][None])
coef = torch.from_numpy(np.stack([st.coef for st in steps]).astype(np.float32)).cuda()
out = torch.empty((S,) + shape, dtype=torch.float32, device="cuda")

ms_a = timed(lambda: T.kspace_mix(buf, coef, out=out), n=500)
nbytes = (K + 2) * 4 * nvox
flops = 2 * (K + 1) * W * nvox
print("(a) kspace_mix alone:            %.3f ms  %d algorithmic bytes  %.3f TB/s  %.2f TFLOP/s fp32"
      % (ms_a, nbytes, nbytes / ms_a / 1e9, flops / ms_a / 1e9))

ms_b = timed(lambda: T.execute({"mri": image}, {}, plans), n=200)
print("(b) Motion step (%d warps + mix): %.3f ms" % (S * K, ms_b))

try:
    freq = np.fft.fftshift(np.arange(W))

    def runs(positions):
        """sorted positions as [start, stop) runs: a slab is one range of the unshifted axis, or two where it wraps"""
        positions = np.sort(positions)
        cuts = np.nonzero(np.diff(positions) > 1)[0] + 1
        return [(int(r[0]), int(r[-1]) + 1) for r in np.split(positions, cuts)]

    # per subject: (image, the ranges of the unshifted last axis that its slab fills)
    fills = [[(m, runs(freq[ini:fin])) for m, ini, fin in sl if fin > ini] for sl in slabs]

    def fft_route():
        spectra = torch.fft.fftn(buf, dim=(-3, -2, -1))
        result = torch.empty_like(spectra[:, 0])
        for i in range(S):
            for m, ranges in fills[i]:
                for lo, hi in ranges:
                    result[i, ..., lo:hi] = spectra[i, m, ..., lo:hi]
        return torch.fft.ifftn(result, dim=(-3, -2, -1)).real

    ref = fft_route()
    torch.cuda.synchronize()
    print("    max |(a) - (c)| = %.3e of max|(c)| = %.3e" % (float((out - ref).abs().max()), float(ref.abs().max())))
    ms_c = timed(fft_route, n=200)
    print("(c) torch.fft route:             %.3f ms  (fftn of %d volumes, slab copy, ifftn, real)" % (ms_c, S * (K + 1)))
    print("(a) / (c) = %.3f" % (ms_a / ms_c))
except Exception as e:  # noqa: BLE001  (torch.fft missing or broken on this build: report, do not hide)
    print("(c) torch.fft route: NOT MEASURED — torch.fft is not usable here: %s: %s" % (type(e).__name__, e))
