"""The cross-entropy / focal kernels (csrc/ce_loss.hip) on one MI355X against the index Dice they share a plan with.  Not collected
by pytest.

    python tests/perf/ce_loss_bench.py [--out FILE]     # every measurement, each in a child process under its own time limit;
                                                        # the RESULT lines go to FILE (default profiles/ce_loss_bench.txt)
    python tests/perf/ce_loss_bench.py --only C:dtype   # one measurement in this process (what the children run)

Setup: N = 2 volumes of 160x192x160, C in {2, 5, 32}, fp32 and bf16 logits, labels uniform over the classes, gamma = 2 with class
weights for (b) and (c) (the focal path: a log and a pow per voxel on top of the softmax).  Device events around `n` back-to-back
calls; the variants take turns window by window in one run (a, a again, b, c, d; five rounds after a warm-up round), a figure is
the best window.  Forward and backward are timed apart.
  a   mri3d_softmax_dice_index_fwd / _bwd, the yardstick (timed twice a round: the distance of its two best windows is the spread)
  b   CE only                       mri3d_softmax_ce_index_fwd / _bwd, dice_weight = 0
  c   Dice + CE fused               the same entry points, dice_weight = ce_weight = 1
  d   what a user had to do before  (a) plus F.cross_entropy(logits, labels.long(), weight) and its autograd backward on the same
                                    device tensors (its time is the sum of the two; GB/s are of the fused pass's bytes)
Algorithmic bytes per voxel: forward C * esz + 1, backward 2 * C * esz + 1, the same for a, b and c.
Conditions: (c) faster than (d); the ratio c / a is reported, and flagged where it exceeds 1 by more than three times the spread
of (a) relative to (a)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, VOL = 2, (160, 192, 160)
WHAT = ["%d:%s" % (C, t) for C in (2, 5, 32) for t in ("fp32", "bf16")]
ROUNDS = 5


def _window(fn, n):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / n


def _rounds(variants, n):
    """{name: [ms per call of each round]}, the variants taking turns; the first round is the warm-up."""
    out = {k: [] for k in variants}
    for r in range(ROUNDS + 1):
        for k, fn in variants.items():
            ms = _window(fn, n)
            if r:
                out[k].append(ms)
    return out


def run(what):
    import ctypes
    import torch
    import torch.nn.functional as F
    from mri_epilepsy_diagnosis_amd import _lib, ops
    C, kind = what.split(":")
    C = int(C)
    dtype, dt, esz = (torch.bfloat16, _lib.BF16, 2) if kind == "bf16" else (torch.float32, _lib.F32, 4)
    L, P, st = _lib.lib(), ops._ptr, ops._stream()
    vox = VOL[0] * VOL[1] * VOL[2]
    nvox = N * vox
    g = torch.Generator().manual_seed(4)
    lab = torch.randint(0, C, (nvox,), generator=g).to(torch.uint8).cuda()
    logits = (3.0 * torch.randn(nvox, C, device="cuda")).to(dtype)
    dlogits = torch.empty_like(logits)
    w = (0.5 + torch.rand(C, generator=g)).cuda()
    loss, dloss = torch.empty(1, device="cuda"), torch.ones(1, device="cuda")
    stats_a, stats_b, stats_c = (torch.empty(4 + N * C * 3, device="cuda") for _ in range(3))
    ga = _lib.DiceIndexGeom(N, vox, C, C, 1e-9, dt)
    gb = _lib.CeIndexGeom(N, vox, C, C, 1e-9, dt, 2.0, 0.0, 1.0)
    gc = _lib.CeIndexGeom(N, vox, C, C, 1e-9, dt, 2.0, 1.0, 1.0)
    ws = ops._workspace(1 << 22, lab.device)
    assert ws.numel() >= max(L.mri3d_softmax_dice_index_workspace_bytes(ctypes.byref(ga)), L.mri3d_softmax_ce_index_workspace_bytes(ctypes.byref(gc)))
    a_fwd = lambda: L.mri3d_softmax_dice_index_fwd(ctypes.byref(ga), P(logits), P(lab), P(loss), P(stats_a), P(ws), ws.numel(), st)   # noqa: E731
    a_bwd = lambda: L.mri3d_softmax_dice_index_bwd(ctypes.byref(ga), P(logits), P(lab), P(stats_a), P(dloss), P(dlogits), st)   # noqa: E731

    def ce(geom, stats):
        return (lambda: L.mri3d_softmax_ce_index_fwd(ctypes.byref(geom), P(logits), P(lab), P(w), P(loss), P(stats), P(ws), ws.numel(), st),
                lambda: L.mri3d_softmax_ce_index_bwd(ctypes.byref(geom), P(logits), P(lab), P(w), P(stats), P(dloss), P(dlogits), st))
    (b_fwd, b_bwd), (c_fwd, c_bwd) = ce(gb, stats_b), ce(gc, stats_c)
    for fn in (a_fwd, a_bwd, b_fwd, b_bwd, c_fwd, c_bwd):
        assert fn() == 0, L.mri3d_last_error()
    # the user's former path: the same memory as an (N, C, D, H, W) tensor, the class map widened to int64 on every call
    x = logits.view(N, *VOL, C).permute(0, 4, 1, 2, 3).requires_grad_(True)
    lab5 = lab.view(N, *VOL)
    held = {}

    def d_fwd():
        a_fwd()
        held["loss"] = F.cross_entropy(x, lab5.long(), weight=w.to(dtype))

    def d_bwd():
        a_bwd()
        torch.autograd.grad(held["loss"], x, retain_graph=True)
    d_fwd()
    n = 40 if C <= 8 else 12
    tf = _rounds({"a": a_fwd, "a2": a_fwd, "b": b_fwd, "c": c_fwd, "d": d_fwd}, n)
    tb = _rounds({"a": a_bwd, "a2": a_bwd, "b": b_bwd, "c": c_bwd, "d": d_bwd}, n)
    for tag, t, per in (("fwd", tf, C * esz + 1), ("bwd", tb, 2 * C * esz + 1)):
        best = {k: min(v) for k, v in t.items()}
        spread = abs(best["a"] - best["a2"])
        ya = min(best["a"], best["a2"])
        for k, name in (("a", "a index Dice"), ("a2", "a index Dice again"), ("b", "b CE only"), ("c", "c Dice + CE fused"), ("d", "d Dice, then torch CE")):
            print("RESULT C=%-2d %s %s  %-22s %8.4f ms  %6.3f TB/s  (%d B/voxel)  windows %s"
                  % (C, kind, tag, name, best[k], per * nvox / best[k] / 1e9, per, " ".join("%.4f" % v for v in t[k])), flush=True)
        ratio = best["c"] / ya
        over = ratio - 1.0 > 3.0 * spread / ya
        print("RESULT C=%-2d %s %s  c / a = %.3f (spread of a %.4f ms = %.3f of a; %s);  b / a = %.3f;  c %s d: %.4f ms against %.4f ms (%.2fx)"
              % (C, kind, tag, ratio, spread, spread / ya, "ABOVE 1 by more than 3 spreads" if over else "within 3 spreads of 1 or below",
                 best["b"] / ya, "faster than" if best["c"] < best["d"] else "NOT FASTER THAN", best["c"], best["d"], best["d"] / best["c"]), flush=True)


if __name__ == "__main__":
    if "--only" in sys.argv:
        run(sys.argv[sys.argv.index("--only") + 1])
        sys.exit(0)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ce_loss_bench.txt")
    lines = []
    for what in WHAT:      # one child at a time; after a child that failed or ran out of time nothing more is started
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", what], timeout=150, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            sys.exit("ce_loss_bench: %s ran past its time limit; stopping" % what)
        got = [line for line in r.stdout.splitlines() if line.startswith("RESULT")]
        sys.stdout.write("".join(line + "\n" for line in got))
        sys.stdout.flush()
        lines += got
        with open(out_path, "w") as f:
            f.write("".join(line + "\n" for line in lines))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            sys.exit("ce_loss_bench: %s ended with status %d; stopping" % (what, r.returncode))
