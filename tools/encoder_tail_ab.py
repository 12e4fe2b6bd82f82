"""Device time of the U-Net's two encoder tails (BatchNorm + PReLU -> skip, MaxPool3d(2)) from rocprofv3 kernel traces of bench.py.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python bench.py --steps 5 --warmup 3 [--dtype bf16]
    python tools/encoder_tail_ab.py f32|bf16 LABEL=DIR [LABEL=DIR ...]

With the two operators (UNet.fused_pool = False, or a build without the fold) the launches that serve a tail are found by their
place in the stream: the norm_act_fwd_kernel launch in front of each maxpool2_fwd_kernel launch, and the norm_act_bwd_reduce /
norm_act_bwd_apply launches behind each maxpool_bwd_kernel launch.  With the fold they are the norm_act_pool_* launches.  The
level (16 channels at 160x192x160, 32 channels at 80x96x80, batch 2) is told by the launch's duration: the two differ fourfold.
Prints, per directory, the mean duration of each kernel and level (first launch of each dropped: cold), their sum per step, and
the achieved GB/s of the fused kernels from the bytes the algorithm needs."""
import csv
import glob
import os
import sys

N, SHAPE = 2, (160, 192, 160)
LEVELS = {"c16": (16, 1), "c32": (32, 2)}     # channels, downsampling of the level's input


def _unit(level, esz):
    c, f = LEVELS[level]
    elems = N * c * (SHAPE[0] // f) * (SHAPE[1] // f) * (SHAPE[2] // f)
    return elems * esz, elems // 8            # bytes of one tensor of the level; index bytes of its pooled tensor


# bytes per launch in units of (tensor, index bytes): read + written
FUSED_BYTES = {"pool_fwd": (2.125, 1), "pool_bwd_sums": (2.125, 1), "pool_bwd_dx": (3.125, 1)}


def _rows(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("%s: expected one *kernel_trace.csv, found %d" % (d, len(files)))
    with open(files[0], newline="") as f:
        rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)]
    rows.sort()
    return rows


def _kind(name):
    if "norm_act_pool_fwd_kernel" in name:
        return "pool_fwd"
    if "norm_act_pool_bwd_kernel" in name:
        # <T, SUMS, DX>: the sums pass is <.., true, false>; the profiler leaves some bf16 instantiations mangled (Lb1E = true)
        args = name.split("norm_act_pool_bwd_kernel", 1)[1].split("(")[0].replace(" ", "")
        return "pool_bwd_sums" if (args.endswith(",false>") or "Lb1ELb0E" in args) else "pool_bwd_dx"
    for key, kind in (("maxpool2_fwd_kernel", "maxpool2_fwd"), ("maxpool_bwd_kernel", "maxpool_bwd"),
                      ("norm_act_bwd_reduce_kernel", "bwd_reduce"), ("norm_act_bwd_apply_kernel", "bwd_apply")):
        if key in name:
            return kind
    if "norm_act_fwd_kernel" in name:
        return "norm_act_fwd"
    return None


def tail_launches(rows):
    """{kind: [duration_ns of every launch that serves an encoder tail]}"""
    kinds = [(_kind(n), dur) for _, dur, n in rows]
    kinds = [(k, dur) for k, dur in kinds if k is not None]
    out = {}
    for i, (k, dur) in enumerate(kinds):
        if k.startswith("pool_"):
            out.setdefault(k, []).append(dur)
        elif k == "maxpool2_fwd":
            out.setdefault(k, []).append(dur)
            j = max(j for j in range(i) if kinds[j][0] == "norm_act_fwd")
            out.setdefault("norm_act_fwd", []).append(kinds[j][1])
        elif k == "maxpool_bwd":
            out.setdefault(k, []).append(dur)
            for want in ("bwd_reduce", "bwd_apply"):
                j = min(j for j in range(i + 1, len(kinds)) if kinds[j][0] == want)
                out.setdefault(want, []).append(kinds[j][1])
    return out


def per_level(durs):
    """{level: mean ns} — the launches split at the geometric middle of the shortest and the longest, the first of each dropped."""
    cut = (min(durs) * max(durs)) ** 0.5
    res = {}
    for level, sel in (("c16", [d for d in durs if d > cut]), ("c32", [d for d in durs if d <= cut])):
        sel = sel[1:] if len(sel) > 1 else sel
        res[level] = (sum(sel) / len(sel), len(sel))
    return res


def main():
    dtype, esz = sys.argv[1], {"f32": 4, "bf16": 2}[sys.argv[1]]
    sums = {}
    for arg in sys.argv[2:]:
        label, d = arg.split("=", 1)
        launches = tail_launches(_rows(d))
        total = {"c16": 0.0, "c32": 0.0}
        print("%s  (%s, %s)" % (label, dtype, d))
        for kind in sorted(launches):
            for level, (ns, cnt) in per_level(launches[kind]).items():
                total[level] += ns
                rate = ""
                if kind in FUSED_BYTES:
                    tb, ib = _unit(level, esz)
                    rate = "  %6.0f GB/s" % ((FUSED_BYTES[kind][0] * tb + FUSED_BYTES[kind][1] * ib) / ns)
                print("  %-14s %s  %8.1f us  (mean of %d launches)%s" % (kind, level, ns / 1e3, cnt, rate))
        print("  per step: c16 %.1f us + c32 %.1f us = %.1f us" % (total["c16"] / 1e3, total["c32"] / 1e3, sum(total.values()) / 1e3))
        sums[label] = total
    return sums


if __name__ == "__main__":
    main()
