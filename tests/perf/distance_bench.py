"""Distance maps on the device (csrc/distance.hip) on one MI355X against what they replace.  Not collected by pytest.

    python tests/perf/distance_bench.py [--out FILE]      # every measurement, each size in a child process under its own time limit;
                                                          # the RESULT lines also go to FILE (default profiles/distance_bench.txt)
    python tests/perf/distance_bench.py --only NAME       # one size in this process (what the children run)

Sizes: 2 x 160x192x160 and 1 x 182x218x182.  Masks (uint8, on the device):
  ribbon   a cortex-like sheet: the 47th..53rd percentile band of Gaussian-filtered noise (sigma 6)
  lesion   one ball of radius 5 (about 500 voxels) in an empty volume: the detector's regime
  noise    every voxel 1 with probability 0.5
Per mask, device events around back-to-back calls after a warm-up window, best of three windows:
  edt_sq            ops.edt_sq of the batch, 500 calls a window: ms per call as issued from Python (three launches), and GB/s of the
                    algorithmic bytes (1 read + 4 written per voxel); then its kernels' own durations from a profiler window
  surface / 2       half of one mri3d_surface_distance(mask, mask) call per volume: that call holds two brute-force transforms of
                    a slightly larger grid plus two cheap passes, so half of it is a generous estimate of what reusing surface.hip's
                    passes would cost.  Bar of the feature: edt_sq is not slower than this on any mask.
  host              mask.cpu() + scipy.ndimage.distance_transform_edt per volume + .cuda(): host clock, best of two
  dilate / erode    radius 3 (ops.edt_threshold: the int32 map is never written)
  signed maps       segmentation.distance.signed_distance_maps(mask as a 2-class map, 2, (1,))
Losses on logits (n, 2, d, h, w) fp32 against the lesion map, forward + backward, same tensors:
  index Dice        ops.softmax_dice_index_loss
  boundary          ops.softmax_boundary_loss on a map made beforehand
  DiceBoundaryLoss  the callable of segmentation/losses.py: signed map + boundary + index Dice
Captured U-Net step (3 levels, 8 first-layer channels, 1 x 160x192x160, fp32; parallel.StepCache replays) with the index Dice,
BoundaryLoss and DiceBoundaryLoss as the loss.  These are recorded, no threshold.
A number that could not be taken is written "not measured".
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIZES = {"2x160x192x160": (2, 160, 192, 160), "1x182x218x182": (1, 182, 218, 182)}
KINDS = ("ribbon", "lesion", "noise")
LIMIT = 420      # seconds per child
PROFILED = 20    # calls under the profiler


def make_mask(kind, shape, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return (rng.random(shape) < 0.5).astype(np.uint8)
    if kind == "lesion":
        g = np.ogrid[:shape[0], :shape[1], :shape[2]]
        c = [int(s * f) for s, f in zip(shape, (0.4, 0.55, 0.6))]
        return (sum((a - b) ** 2 for a, b in zip(g, c)) <= 25).astype(np.uint8)
    from scipy import ndimage
    f = ndimage.gaussian_filter(rng.standard_normal(shape).astype(np.float32), 6.0)
    lo, hi = np.percentile(f, [47, 53])
    return ((f > lo) & (f < hi)).astype(np.uint8)


def windows(fn, n, repeats=3):
    """ms per call: the best of `repeats` windows of n back-to-back calls between device events, after a warm-up window."""
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
    return min(out)


def kernel_times(fn):
    """name -> ms per call of every edt kernel fn() launches (the w pass; the h and d passes together), from the torch profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(PROFILED):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and "edt_" in e.name:
            name = e.name.split("(")[0].split("::")[-1]
            out[name] = out.get(name, 0.0) + e.device_time_total / 1e3 / PROFILED
    return out


def wall(fn, reps):
    import torch
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def say(tag, what, text):
    print("RESULT %-14s %-8s %s" % (tag, what, text), flush=True)


def run(name):
    import numpy as np
    import torch
    from scipy import ndimage
    from mri_epilepsy_diagnosis_amd import ops, parallel
    from mri_epilepsy_diagnosis_amd.segmentation import distance, losses, surface
    from mri_epilepsy_diagnosis_amd.unet import UNet
    n, d, h, w = SIZES[name]
    nvox = n * d * h * w
    masks = {}
    for kind in KINDS:
        host = np.stack([make_mask(kind, (d, h, w), 10 * i + 1) for i in range(n)])
        m = torch.from_numpy(host).cuda()
        masks[kind] = m
        out = torch.empty(m.shape, dtype=torch.int32, device="cuda")
        u8 = torch.empty(m.shape, dtype=torch.uint8, device="cuda")
        t_edt = windows(lambda: ops.edt_sq(m, out=out), 500)
        t_surf = windows(lambda: surface.surface_distance_sums(m[0], m[0]), 10) * n / 2
        say(name, kind, "edt_sq %8.3f ms  %7.1f GB/s   surface / 2 %8.3f ms   %s (%.1fx)"
            % (t_edt, 5.0 * nvox / t_edt / 1e6, t_surf, "bar met" if t_edt <= t_surf else "BAR MISSED", t_surf / t_edt))

        def host_route():
            hm = m.cpu().numpy()
            return torch.from_numpy(np.stack([ndimage.distance_transform_edt(v) for v in hm]).astype(np.float32)).cuda()
        t_host = wall(host_route, 2)
        say(name, kind, "host route (cpu + scipy + cuda) %9.1f ms: the device transform is %.0fx faster" % (t_host, t_host / t_edt))
        say(name, kind, "dilate r=3 %8.3f ms   erode r=3 %8.3f ms   signed maps ids (1,) %8.3f ms"
            % (windows(lambda: distance.dilate(m, 3, out=u8), 300), windows(lambda: distance.erode(m, 3, out=u8), 300),
               windows(lambda: distance.signed_distance_maps(m, 2, (1,)), 200)))
        say(name, kind, "edt_sq kernels (profiler, mean of %d calls): %s" % (PROFILED, "   ".join("%s %.3f ms" % kv for kv in kernel_times(lambda: ops.edt_sq(m, out=out)).items())))
    # losses on the lesion map
    y = masks["lesion"]
    logits = torch.randn((n, 2, d, h, w), device="cuda").contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    smap = ops.signed_sqdist(y, 2, (1,))
    both = losses.DiceBoundaryLoss(1.0, 1.0, (1,), 2)

    def fb(loss_of):
        def step():
            logits.grad = None
            loss_of().backward()
        return windows(step, 100)
    say(name, "losses", "fwd + bwd: index Dice %8.3f ms   boundary %8.3f ms   DiceBoundaryLoss (maps included) %8.3f ms"
        % (fb(lambda: ops.softmax_dice_index_loss(logits, y)), fb(lambda: ops.softmax_boundary_loss(logits, smap, (1,))),
           fb(lambda: both(logits, y))))
    if name != "2x160x192x160":
        return
    torch.manual_seed(0)
    model = UNet(in_channels=1, out_classes=2, dimensions=3, num_encoding_blocks=3, out_channels_first_layer=8, normalization="batch",
                 upsampling_type="linear", padding=True, activation="PReLU").cuda()
    x = torch.randn((1, 1, d, h, w), device="cuda")
    t = y[:1].contiguous()
    cache = parallel.StepCache.of(model)
    steps = {}
    for label, fn in (("index Dice", ops.softmax_dice_index_loss), ("BoundaryLoss", losses.BoundaryLoss((1,), 2)), ("DiceBoundaryLoss", both)):
        steps[label] = windows(lambda: cache.run(x, t, fn, backward=True), 20)
    say(name, "unet", "captured step 1 x %dx%dx%d: %s   (captures %d, eager runs %d)"
        % (d, h, w, "   ".join("%s %8.3f ms" % kv for kv in steps.items()), cache.captures, cache.eager_runs))


if __name__ == "__main__":
    if "--only" in sys.argv:
        run(sys.argv[sys.argv.index("--only") + 1])
        sys.exit(0)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "distance_bench.txt")
    lines = []
    status = 0
    for name in SIZES:       # one child at a time; after a child that failed or ran out of time nothing more is started
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", name], timeout=LIMIT, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            lines.append("RESULT %-14s not measured: ran past its time limit of %d s" % (name, LIMIT))
            status = "distance_bench: %s ran past its time limit; stopping" % name
            break
        lines += [line for line in r.stdout.splitlines() if line.startswith("RESULT")]
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            lines.append("RESULT %-14s not measured beyond this line: the run ended with status %d" % (name, r.returncode))
            status = "distance_bench: %s ended with status %d; stopping" % (name, r.returncode)
            break
    text = "".join(line + "\n" for line in lines)
    sys.stdout.write(text)
    with open(out_path, "w") as f:
        f.write(text)
    sys.exit(status)
