"""Affine registration to the template (csrc/register.hip, mri_epilepsy_diagnosis_amd/registration) on one MI355X.  Not collected by
pytest.

    python tests/perf/registration_bench.py [--out profiles/registration_bench.txt] [--no-cpu]

Workload: the grey-matter template grid (tests/golden/mni152_gm_u8.npz, 182x218x182) as the fixed volume, counted where it is
non-zero, and a synthetic moving volume made from it: the template seen through a known 12-parameter transform on a 176x208x176
grid, with a monotone intensity change and smooth noise added.  Per pyramid level (4 levels) one joint_hist call is timed for
k = 1, 24 and 64 candidates scattered about the true matrix: device events around n back-to-back calls after a warm-up window,
three windows, the best one reported (the spread beside it).  A sample is one (candidate, counted fixed voxel) pair.  Algorithmic
bytes per call: the fixed bytes once per candidate group (the kernel's unit of reuse) plus the moving volume once per candidate,
4 bytes a voxel; bytes/s is that over the call time, an end-to-end figure of the three launches, not a kernel's share of peak.
Level 0 is also timed for k = 24 with nothing skipped, and on two substitute moving volumes that bracket the same-address LDS
contention (uniform noise: samples spread over all bins; a constant: all in one bin) with unchanged coordinates and gathers.
A full 12-dof `register` is wall clock around a device synchronise (it crosses to the host once per search call), run twice,
the second reported.  The host restatement is one evaluation of the same cost on this machine's CPU:
scipy.ndimage.affine_transform (order 1) + np.histogram2d.  There is no bar: the path is new."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MOVING_SHAPE, BINS, LEVELS = (176, 208, 176), 64, 4
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
    from mri_epilepsy_diagnosis_amd import _lib, ops, registration

    L, P, st = _lib.lib(), ops._ptr, ops._stream()
    gm = np.load(os.path.join(ROOT, "tests", "golden", "mni152_gm_u8.npz"))["gm"]
    fixed = torch.from_numpy(gm.astype(np.float32)).cuda()
    fshape = tuple(fixed.shape)
    truth_p = np.array([3.0, -4.0, 2.5] + list(np.deg2rad([5.0, -4.0, 6.0])) + [0.05, -0.04, 0.03, 0.02, -0.015, 0.01])
    truth = registration.params_to_matrix(truth_p, fshape, MOVING_SHAPE)
    # moving(m) = template(truth^-1 m), then a monotone intensity change and smooth noise
    seen = registration.apply(fixed, registration.invert(truth), MOVING_SHAPE)
    g = torch.Generator(device="cuda").manual_seed(0)
    noise = torch.randn(tuple((s + 1) // 2 for s in MOVING_SHAPE), generator=g, device="cuda")
    noise = torch.nn.functional.interpolate(noise[None, None], size=MOVING_SHAPE, mode="trilinear")[0, 0]
    moving = (255.0 * (seen / 255.0) ** 0.7 + 6.0 * noise).contiguous()
    mask = fixed > 0
    say("device %s; fixed %dx%dx%d (%d voxels, %d counted), moving %dx%dx%d, %d bins"
        % ((torch.cuda.get_device_name(0),) + fshape + (fixed.numel(), int(mask.sum())) + MOVING_SHAPE + (BINS,)))

    pf, pm = registration.Pyramid(fixed, LEVELS), registration.Pyramid(moving, LEVELS)
    masks = [mask]
    for _ in range(LEVELS - 1):
        masks.append(ops.downsample2(masks[-1].float()) >= 0.5)
    rng = np.random.default_rng(0)
    scatter = [truth_p] + [truth_p + rng.uniform(-1, 1, 12) * registration.step_vector(2.0, 12) for _ in range(63)]
    for level in range(LEVELS):
        f_lo, f_scale = pf.scale(level, BINS)
        m_lo, m_scale = pm.scale(level, BINS)
        mov = pm.volumes[level]
        for skip in ((True, False) if level == 0 else (True,)):
            fb = ops.quantize_bins(pf.volumes[level], f_lo, f_scale, BINS, mask=masks[level] if skip else None)
            counted = int((fb != 255).sum())
            for k in ((1, 24, 64) if skip else (24,)):
                mats = np.stack([registration.level_matrix(registration.params_to_matrix(p, fshape, MOVING_SHAPE), level) for p in scatter[:k]])
                aff = torch.from_numpy(mats).to(device="cuda", dtype=torch.float32).contiguous()
                hist = torch.empty((k, BINS, BINS), dtype=torch.int64, device="cuda")
                need = L.mri3d_joint_hist_workspace_bytes(*fb.shape, k, BINS)
                ws = ops._workspace(need, fb.device)
                plan = ops.joint_hist_plan(fb.shape, k, BINS)
                call = lambda: L.mri3d_joint_hist(P(fb), *fb.shape, P(mov), *mov.shape, P(aff), k, m_lo, m_scale, BINS, P(hist), P(ws),  # noqa: E731
                                                  ws.numel(), st)
                w = windows(call, 20 if level == 0 else 100)
                ms = min(w)
                nbytes = plan["groups"] * fb.numel() + k * 4 * mov.numel()
                inside = int(hist.sum()) / max(k * counted, 1)
                say("RESULT joint_hist level %d %3dx%3dx%3d %s k %2d   %.4f ms  (windows %s)  %.3e samples/s  %.3f TB/s algorithmic  "
                    "(%d blocks x %d groups, %d trips, %.1f %% of samples inside)"
                    % ((level,) + tuple(fb.shape) + ("masked  " if skip else "unmasked", k, ms, " ".join("%.4f" % v for v in w),
                                                    k * counted / (ms * 1e-3), nbytes / ms / 1e9, plan["blocks"], plan["groups"], plan["trips"],
                                                    100.0 * inside)))

    # same-address LDS contention: the same launch (same coordinates, same gathers) on moving volumes whose samples spread over all
    # bins (uniform noise) or all fall into one bin (a constant), beside the synthetic volume
    f_lo, f_scale = pf.scale(0, BINS)
    m_lo, m_scale = pm.scale(0, BINS)
    k = 24
    mats = np.stack([registration.params_to_matrix(p, fshape, MOVING_SHAPE) for p in scatter[:k]])
    aff = torch.from_numpy(mats).to(device="cuda", dtype=torch.float32).contiguous()
    hist = torch.empty((k, BINS, BINS), dtype=torch.int64, device="cuda")
    span = BINS / m_scale
    variants = (("synthetic", moving), ("uniform noise", (m_lo + span * torch.rand(MOVING_SHAPE, generator=g, device="cuda")).contiguous()),
                ("constant", torch.full(MOVING_SHAPE, m_lo + 0.5 * span, device="cuda")))
    for skip in (True, False):
        fb = ops.quantize_bins(fixed, f_lo, f_scale, BINS, mask=mask if skip else None)
        ws = ops._workspace(L.mri3d_joint_hist_workspace_bytes(*fb.shape, k, BINS), fb.device)
        for name, mov in variants:
            call = lambda: L.mri3d_joint_hist(P(fb), *fb.shape, P(mov), *mov.shape, P(aff), k, m_lo, m_scale, BINS, P(hist), P(ws),  # noqa: E731
                                              ws.numel(), st)
            w = windows(call, 20)
            say("RESULT contention level 0 %s k %d moving = %-13s  %.4f ms  (windows %s)  %d cells of %d non-zero"
                % ("masked  " if skip else "unmasked", k, name, min(w), " ".join("%.4f" % v for v in w), int((hist != 0).sum()), hist.numel()))

    for attempt in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = registration.register(moving, fixed, fixed_mask=mask, dof=12, bins=BINS, levels=LEVELS)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    say("RESULT register 12 dof, %d levels   %.3f s wall  (%s evaluations in %s calls per level, coarsest first); corner displacement "
        "from the truth %.3f voxels, cost %.5f, overlap %d"
        % (LEVELS, wall, [t["evaluations"] for t in res.trace], [t["calls"] for t in res.trace],
           registration.corner_displacement(res.matrix, truth, fshape), res.cost, res.overlap))

    if "--no-cpu" not in sys.argv:
        from scipy import ndimage
        h_fixed, h_moving, h_mask = fixed.cpu().numpy(), moving.cpu().numpy(), mask.cpu().numpy()
        f_lo, f_scale = pf.scale(0, BINS)
        m_lo, m_scale = pm.scale(0, BINS)
        t0 = time.perf_counter()
        warped = ndimage.affine_transform(h_moving, truth[:, :3], truth[:, 3], fshape, order=1, mode="constant", cval=np.nan)
        ok = h_mask & np.isfinite(warped)
        bf = np.clip(np.floor((h_fixed[ok] - f_lo) * f_scale), 0, BINS - 1)
        bm = np.clip(np.floor((warped[ok] - m_lo) * m_scale), 0, BINS - 1)
        H, _, _ = np.histogram2d(bf, bm, bins=BINS, range=[[0, BINS], [0, BINS]])
        cpu_s = time.perf_counter() - t0
        dev = ops.joint_histogram(ops.quantize_bins(fixed, f_lo, f_scale, BINS, mask=mask), moving, truth, m_lo, m_scale, BINS)[0].cpu().numpy()
        say("RESULT cpu: scipy %s affine_transform + np.histogram2d, one evaluation at level 0   %.2f s on this machine's CPU; "
            "%d samples against the device's %d, %d of them in another bin"
            % (__import__("scipy").__version__, cpu_s, int(H.sum()), int(dev.sum()), int(np.abs(H - dev).sum() // 2)))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
