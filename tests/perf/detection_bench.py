"""The detection path (csrc/detection.hip, mri_epilepsy_diagnosis_amd/detection) on one MI355X, beside the numpy restatement on
the box's host.  Not collected by pytest.  No bars: the path is new, there is no earlier time to hold it to.

    python tests/perf/detection_bench.py                 # every measurement, each in a child process under its own time limit
    python tests/perf/detection_bench.py --only NAME     # one measurement in this process (what the children run)

Setup: the MNI152 grey-matter template of tests/golden (182 x 218 x 182), h = 16, w = 32: 5230 patches of 2 x 16 x 32.  Device
events around `n` back-to-back calls after a warm-up window, three windows; a figure is the best window.  Bytes are algorithmic:
  gather   4 B read + 4 B written per patch element (5230 x 1024 elements)
  paint    1 B written per voxel (the patch map and the starts are a few KB)
  plan     wall clock of PatchPlan(gm): two launches, two small copies to the host and the table loop in Python
  forward  PatchModel in eval mode over all patches in batches of 512, channels-last patches
  host     tests/detection_ref.py on the CPU, wall clock, best of 3
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 16, 32
WHAT = ["plan", "gather", "forward", "vote_paint", "host"]


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


def wall(fn, repeats=3):
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def _setup():
    import numpy as np
    import torch
    from util import load_golden
    gm = load_golden("mni152_gm_u8.npz")["gm"]
    vol = np.random.default_rng(0).random(gm.shape, dtype=np.float32)
    return gm, vol, torch.from_numpy(gm).cuda(), torch.from_numpy(vol).cuda()


def report(name, ms, nbytes=None):
    rate = "" if nbytes is None else "  %.1f GB/s" % (nbytes / ms / 1e6)
    print("RESULT %-44s %.4f ms%s" % (name, ms, rate), flush=True)


def run(what):
    import numpy as np
    import torch
    import detection_ref as R
    from mri_epilepsy_diagnosis_amd.detection import FCDMaskGenerator, PatchModel, mask as dmask, patches
    gm, vol, gm_d, vol_d = _setup()
    if what == "host":
        report("host: strip starts + table", wall(lambda: R.base_table(gm, H, W)))
        table, kinds = R.base_table(gm, H, W)
        report("host: gather of %d patches" % len(table), wall(lambda: R.gather(vol, table, H, W)))
        m = R.map_of_labels((np.arange(len(table)) % 3 != 0).astype(np.uint8), gm, H, W)
        report("host: vote + paint", wall(lambda: R.paint(R.vote(m), gm, H, W)))
        return
    def sync_plan():
        p = patches.PatchPlan(gm_d, H, W)
        torch.cuda.synchronize()
        return p
    plan = sync_plan()
    nelem = len(plan) * 2 * H * W
    if what == "plan":
        report("plan (PatchPlan, wall clock)", wall(sync_plan))
        gm_f = gm_d.float()
        report("strip_starts, all %d row offsets (with the sign check)" % (gm.shape[1] - H + 1),
               min(windows(lambda: patches.strip_starts(gm_f, H), 20)))
    elif what == "gather":
        for cl in (False, True):
            for order in (plan.order, None):
                fn = lambda: patches.mirror_patches(vol_d, plan.table, H, W, cl, order)   # noqa: E731
                report("gather %d patches, %s, %s" % (len(plan), "channels last" if cl else "NCHW", "sorted work order" if order is not None else "table order"),
                       min(windows(fn, 50)), 8 * nelem)
    elif what == "forward":
        torch.manual_seed(0)
        gen = FCDMaskGenerator(PatchModel(), plan, batch_size=512)
        gen.predict_labels(vol_d)
        report("gather + batched forward + arg-max (batch 512)", min(windows(lambda: gen.predict_labels(vol_d), 3)))
    elif what == "vote_paint":
        labels = torch.from_numpy((np.arange(len(plan)) % 3 != 0).astype(np.uint8)).cuda()
        gen = FCDMaskGenerator(PatchModel(), plan)
        m = gen.map_of_labels(labels)
        report("vote [4, 13, 182]", min(windows(lambda: dmask.patch_vote(m), 200)))
        report("paint 182 x 218 x 182", min(windows(lambda: gen.masking(m), 200)), gm.size)
        report("vote + paint", min(windows(lambda: gen.masking(gen.postprocess(m)), 200)), gm.size)
    else:
        sys.exit("detection_bench: unknown measurement %s" % what)


if __name__ == "__main__":
    if "--only" in sys.argv:
        run(sys.argv[sys.argv.index("--only") + 1])
        sys.exit(0)
    for what in WHAT:      # one child at a time; after a child that failed or ran out of time nothing more is started
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", what], timeout=180, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            sys.exit("detection_bench: %s ran past its time limit; stopping" % what)
        sys.stdout.write("".join(line + "\n" for line in r.stdout.splitlines() if line.startswith("RESULT")))
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            sys.exit("detection_bench: %s ended with status %d; stopping" % (what, r.returncode))
