"""The case table of the cross-entropy / focal suites (tests/test_ce_ref.py, tests/test_ce_plan.py, tests/test_ce_loss_gpu.py).

A row: C, spatial size, storage type, label kind, weights, gamma, logit scale, pitch (None: dense), the two loss weights, and the
corner of the launch plan the row is there for, which test_ce_plan.py holds it to through ops.ce_index_plan:
    bucket   class bucket 2 / 4 / 8 / 16 / 32
    mode     "scalar" (element by element), "rows4" (a voxel's classes in 4-element vectors), "vox4" (two dense classes, 4 voxels a lane)
    fwd      "partial": one block whose last trip is a partial one, at most one whole trip before it;  "trips": at least two whole
             trips, the loop goes round with every lane busy
    bwd      "partial": no whole trip;  "trips": 2048 blocks, at least one whole trip and a partial one
Plan rules (csrc/loss_index.h, the index Dice's): forward min(ceil(items / 1024), 2048 / N) blocks of 256 lanes per sample,
backward min(ceil(items / 256), 2048, 4096 / N); items = voxels, or for vox4 the 4-voxel groups and the single voxels around them.
5x7x9 = 315 voxels: one block, 256 + 59 voxels, and for C = 2 81 items, head and tail singles beside the groups.  7x11x37 = 2849 voxels: 3
blocks, three whole forward trips (C = 2: one block, two).  The backward goes round only above 524 288 items: 81^3 for C > 2,
129^3 for two dense classes, both odd."""
from collections import namedtuple

import torch

from loss_cases import labels_of

BF, F32 = torch.bfloat16, torch.float32
SMALL, TRIPS = (5, 7, 9), (7, 11, 37)
BWD_TRIPS = {2: (129, 129, 129), 3: (81, 81, 81), 8: (81, 81, 81), 9: (81, 81, 81), 17: (81, 81, 81)}
GAMMAS = (0.0, 1.0, 2.0, 3.5)
WEIGHTS = ("none", "ones", "random", "zero_one")
KINDS = ("ignored", "absent", "single", "sample_ignored", "all_ignored")
PITCHED = [(2, 5), (2, 4), (5, 8), (8, 12), (8, 11), (12, 12), (20, 24), (32, 40)]        # tests/test_labels_gpu.py's pairs
CE_ONLY, COMPOUND = (0.0, 1.0), (0.7, 1.3)                                               # (dice_weight, ce_weight)

Case = namedtuple("Case", "group C spatial dtype kind weights gamma scale pitch dice_weight ce_weight corner seed")


def bucket_of(C):
    return 2 if C <= 2 else 4 if C <= 4 else 8 if C <= 8 else 16 if C <= 16 else 32


def mode_of(C, pitch):
    ld = C if pitch is None else pitch
    return "vox4" if C == 2 and ld == 2 else "rows4" if C % 4 == 0 and ld % 4 == 0 else "scalar"


def _case(group, k, C, spatial, dtype, kind, comp, pitch=None, scale=3.0, fwd="partial", bwd="partial", gamma=None, weights=None):
    corner = dict(bucket=bucket_of(C), mode=mode_of(C, pitch), dice=int(comp[0] > 0), fwd=fwd, bwd=bwd)
    return Case(group, C, spatial, dtype, kind, WEIGHTS[k % 4] if weights is None else weights,
                GAMMAS[(k // 2) % 4] if gamma is None else gamma, scale, pitch, comp[0], comp[1], corner, 5000 + 37 * k + C)


def _build():
    rows, k = [], 0

    def add(*a, **kw):
        nonlocal k
        rows.append(_case(a[0], k, *a[1:], **kw))
        k += 1
    # every class count of the index Dice's suite, and 4 and 5 for the rows4 form of bucket 4 and the scalar form of bucket 8
    for C in (2, 3, 4, 5, 8, 9, 12, 17, 20, 32):
        for dtype in (F32, BF):
            for comp in (CE_ONLY, COMPOUND):
                add("base", C, SMALL, dtype, "mixed", comp)
    for C in (2, 3, 8, 9, 17, 32):                                      # the forward loop of every bucket goes round
        for dtype in (F32, BF):
            add("fwd_trips", C, TRIPS, dtype, "ignored", COMPOUND if dtype == F32 else CE_ONLY, fwd="trips")
    for kind in KINDS:
        for C in (2, 5, 32):
            for comp in (CE_ONLY, COMPOUND):
                add("kinds", C, SMALL, F32 if (k // 2) % 2 == 0 else BF, kind, comp)
    for C in (2, 5, 32):                                                # pt rounds to 1 and to 0
        for dtype in (F32, BF):
            for comp in (CE_ONLY, COMPOUND):
                add("confident", C, SMALL, dtype, "ignored", comp, scale=32.0)
    for C, ld in PITCHED:
        for dtype in (F32, BF):
            for comp in (CE_ONLY, COMPOUND):
                add("pitched", C, SMALL, dtype, "ignored", comp, pitch=ld)
    for C in (2, 3, 8, 9, 17):                                          # the backward loop of every bucket goes round
        for dtype in (F32, BF):                                         # (bf16-valued logits: the two share a float64 reference)
            rows.append(_case("bwd_trips", k, C, BWD_TRIPS[C], dtype, "ignored", COMPOUND, fwd="trips", bwd="trips", gamma=2.0,
                              weights="random")._replace(seed=7000 + C))
        k += 1
    return rows


CASES = _build()


def case_id(c):
    return "%s-C%d-%s-%s-%s-w_%s-g%g-s%g%s-%s" % (c.group, c.C, "x".join(map(str, c.spatial)), "bf16" if c.dtype == BF else "f32", c.kind,
                                                    c.weights, c.gamma, c.scale, "" if c.pitch is None else "-ld%d" % c.pitch,
                                                    "dice+ce" if c.dice_weight else "ce")


def group(name):
    return [c for c in CASES if c.group == name]


def weights_of(name, C, seed):
    if name == "none":
        return None
    if name == "ones":
        return torch.ones(C)
    w = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed))
    if name == "zero_one":
        w[1] = 0.0
    return w


def class_map_of(kind, C, spatial, seed):
    if kind in ("mixed", "ignored", "absent", "single"):
        return labels_of(kind, C, spatial, seed)
    lab = labels_of("ignored", C, spatial, seed)
    if kind == "sample_ignored":
        lab[1] = 255
    else:
        lab[:] = C
        lab[0, 0, 0, :3] = 255
    return lab


def inputs_of(c, dtype=None):
    """(logits (2, C, D, H, W) in the storage type on the CPU, class map uint8 (2, D, H, W), weights float32 [C] or None)."""
    z = c.scale * torch.randn(2, c.C, *c.spatial, generator=torch.Generator().manual_seed(c.seed))
    return z.to(c.dtype if dtype is None else dtype), class_map_of(c.kind, c.C, c.spatial, c.seed + 1), weights_of(c.weights, c.C, c.seed + 2)
