"""Connected components on the device (csrc/components.hip) on one MI355X against the host path they replace.  Not collected by pytest.

    python tests/perf/components_bench.py                 # every measurement, each in a child process under its own time limit
    python tests/perf/components_bench.py --only NAME     # one measurement in this process (what the children run)

Setup: one 160x192x160 uint8 mask on the device, of two kinds:
  blobs       Gaussian-filtered noise (sigma 4) thresholded at its 92nd percentile: a few hundred smooth components
  bernoulli   every voxel 1 with probability 0.3: dust under 6-connectivity, one giant cluster and dust under 26
For each mask and each of the 6- and 26-neighbourhoods:
  label           ops.label_components                       device events around 500 back-to-back calls, best of three windows
  label + stats   ops.label_components + one read of the count + ops.component_stats
                                                             host clock around 100 calls ending in a synchronise, best of five
  lesion_scores   segmentation.components.lesion_scores(mask, other mask of the same kind), its host reads included
                                                             host clock around 50 calls, best of five
  phases          each of the six launches of the labelling: the kernel durations the torch profiler records, mean of 20 calls
                  (a run under the profiler, after the timings above)
  host            what this replaces, on the same box: mask.cpu() + scipy.ndimage.label + np.bincount + the int32 label volume
                  copied back to the device                  host clock, best of three single calls
Bar of the feature: `label + stats` on the device is faster than `host` on both masks and both neighbourhoods.
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

VOL = (160, 192, 160)
WHAT = ["blobs", "bernoulli"]
LIMIT = 240      # seconds per child
PROFILED = 20    # calls under the profiler; a phase is its kernel's mean duration over them


def make_mask(kind, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    if kind == "bernoulli":
        return (rng.random(VOL) < 0.3).astype(np.uint8)
    from scipy import ndimage
    f = ndimage.gaussian_filter(rng.standard_normal(VOL).astype(np.float32), 4.0)
    return (f > np.percentile(f, 92)).astype(np.uint8)


def windows(fn, n, repeats=3):
    """ms per call of `repeats` windows of n back-to-back calls, after a warm-up window."""
    import torch
    out = []
    for r in range(repeats + 1):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        if r:
            out.append(start.elapsed_time(stop) / n)
    return out


def wall(fn, reps, n=1):
    """ms per call: the best of `reps` host-clock windows of n calls that end in a device synchronise, after a warm-up call."""
    import torch
    best = float("inf")
    fn()
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t) / n)
    return best * 1e3


def run(kind):
    import numpy as np
    import torch
    from scipy import ndimage
    from torch.profiler import ProfilerActivity, profile
    from mri_epilepsy_diagnosis_amd import ops
    from mri_epilepsy_diagnosis_amd.segmentation import components
    mask_h, other_h = make_mask(kind, 1), make_mask(kind, 2)
    mask, other = torch.from_numpy(mask_h).cuda(), torch.from_numpy(other_h).cuda()
    out = torch.empty(VOL, dtype=torch.int32, device="cuda")
    for conn in (6, 26):
        tag = "%s / %d" % (kind, conn)
        count = int(ops.label_components(mask, conn, out=out)[1])
        w = windows(lambda: ops.label_components(mask, conn, out=out), 500)
        print("RESULT %-18s label                 %8.3f ms   (%d components; windows %s)" % (tag, min(w), count, " ".join("%.3f" % v for v in w)), flush=True)

        def label_stats():
            labels, k = ops.label_components(mask, conn, out=out)
            return ops.component_stats(labels, max(int(k), 1))
        dev = wall(label_stats, 5, 100)
        print("RESULT %-18s label + stats         %8.3f ms" % (tag, dev), flush=True)
        print("RESULT %-18s lesion_scores         %8.3f ms" % (tag, wall(lambda: components.lesion_scores(mask, other, conn), 5, 50)), flush=True)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(PROFILED):
                ops.label_components(mask, conn, out=out)
            torch.cuda.synchronize()
        phases = {}
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA and "cc_" in e.name:
                name = e.name.split("(")[0].split("::")[-1]
                phases[name] = phases.get(name, 0.0) + e.device_time_total / 1e3 / PROFILED
        print("RESULT %-18s phases                %s" % (tag, "  ".join("%s %.3f ms" % p for p in phases.items())), flush=True)

        def host():
            m = mask.cpu().numpy()
            lab, k = ndimage.label(m, structure=ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
            sizes = np.bincount(lab.ravel(), minlength=k + 1)
            return torch.from_numpy(lab.astype(np.int32, copy=False)).cuda(), sizes
        hst = wall(host, 3)
        print("RESULT %-18s host path             %8.3f ms   %s: device label + stats is %.1fx faster"
              % (tag, hst, "bar met" if dev < hst else "BAR MISSED", hst / dev), flush=True)


if __name__ == "__main__":
    if "--only" in sys.argv:
        run(sys.argv[sys.argv.index("--only") + 1])
        sys.exit(0)
    for what in WHAT:      # one child at a time; after a child that failed or ran out of time nothing more is started
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", what], timeout=LIMIT, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            sys.exit("components_bench: %s ran past its time limit; stopping" % what)
        sys.stdout.write("".join(line + "\n" for line in r.stdout.splitlines() if line.startswith("RESULT")))
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            sys.exit("components_bench: %s ended with status %d; stopping" % (what, r.returncode))
