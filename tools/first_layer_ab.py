"""Device time of the U-Net's first layer (Conv3d(1, 8, 3, padding=1) + PReLU, no normalisation) from rocprofv3 kernel traces
of bench.py.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python bench.py --steps 5 --warmup 3
    python tools/first_layer_ab.py LABEL=DIR [LABEL=DIR ...]

With the four launches (UNet.fused_first = False, or a build without the fold) the layer is conv_cin1_fwd_kernel, the
norm_act_fwd_kernel launch behind it, norm_act_bwd_frozen_kernel (the step's only activation-only backward) and
conv_cin1_wgrad_kernel.  With the fold it is conv_cin1_act_fwd_kernel and conv_cin1_act_bwd_kernel.  Prints, per directory, the
mean duration of each launch (the first of each dropped: cold), the smallest and largest, the achieved GB/s from the bytes the
algorithm needs, and the sum per step."""
import csv
import glob
import os
import sys

CV = 2 * 160 * 192 * 160 * 4     # bytes of one channel-volume of the bench step (batch 2, fp32)
# channel-volumes read + written per launch
BYTES = {"cin1_fwd": 9, "act_fwd": 16, "act_bwd_frozen": 24, "cin1_wgrad": 9, "cin1_act_fwd": 17, "cin1_act_bwd": 17}


def _rows(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("%s: expected one *kernel_trace.csv, found %d" % (d, len(files)))
    with open(files[0], newline="") as f:
        rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)]
    rows.sort()
    return rows


def first_layer_launches(rows):
    """{kind: [duration_ns of every launch that serves the first layer]}"""
    out = {}
    for i, (_, dur, name) in enumerate(rows):
        if "conv_cin1_act_fwd_kernel" in name:
            out.setdefault("cin1_act_fwd", []).append(dur)
        elif "conv_cin1_act_bwd_kernel" in name:
            out.setdefault("cin1_act_bwd", []).append(dur)
        elif "conv_cin1_fwd_kernel" in name:
            out.setdefault("cin1_fwd", []).append(dur)
            j = min(j for j in range(i + 1, len(rows)) if "norm_act_fwd_kernel" in rows[j][2])
            out.setdefault("act_fwd", []).append(rows[j][1])
        elif "conv_cin1_wgrad_kernel" in name:
            out.setdefault("cin1_wgrad", []).append(dur)
        elif "norm_act_bwd_frozen_kernel" in name:
            out.setdefault("act_bwd_frozen", []).append(dur)
    return out


def main():
    sums = {}
    for arg in sys.argv[1:]:
        label, d = arg.split("=", 1)
        launches = first_layer_launches(_rows(d))
        total = 0.0
        print("%s  (%s)" % (label, d))
        for kind in sorted(launches):
            sel = launches[kind][1:] if len(launches[kind]) > 1 else launches[kind]
            ns = sum(sel) / len(sel)
            total += ns
            print("  %-15s %8.1f us  (mean of %d launches, %.1f .. %.1f)  %6.0f GB/s"
                  % (kind, ns / 1e3, len(sel), min(sel) / 1e3, max(sel) / 1e3, BYTES[kind] * CV / ns))
        print("  per step: %.1f us" % (total / 1e3))
        sums[label] = total
    return sums


if __name__ == "__main__":
    main()
