"""Rows of the fused-convolution parity suite (tests/test_fusedconv_parity_gpu.py; their meaning: tests/fusedconv_run.py).

UpRow    Conv3d over a nearest-upsampled input (csrc/upconv.hip), all three passes:
  id       names the (Ci, Co, taps) instance and the scale: with the storage type of the test id, the 6 kernels the row launches
  ci, co   channels;  k  kernel;  S  scale;  sp  COARSE extents;  pad  padding;  n  batch
  layout   {"x" | "y": (channels of the wider buffer, first channel of the slice)}: x also places dx, y also places dy
  bias, dbias   False: the NULL pointer
  nums     {"fwd" | "dgrad" | "wgrad": {field of ops.upconv_plan: value}}: the plan numbers the row is there for
PairRow  the first convolution's weight gradient through the second (csrc/sepconv.hip):
  sp       extents (D, H, W) of x;  s1, p1  the first convolution (6 taps along D);  k2, s2, p2  the second (along H)
  layout   {"x" | "dy2": (channels, first channel)};  dbias  False: dbias1 = NULL;  nums  {field of ops.conv_pair_plan: value}"""
import collections

UpRow = collections.namedtuple("UpRow", "id ci co k S sp pad n layout bias dbias nums")
PairRow = collections.namedtuple("PairRow", "id n sp s1 p1 k2 s2 p2 layout dbias nums")

DTYPES = ("f32", "bf16")
INSTANCES = [(8, 1, 3), (8, 2, 3), (4, 1, 3), (4, 2, 3), (4, 4, 3), (16, 1, 3), (8, 1, 6), (4, 1, 6), (4, 2, 6),
             (8, 1, 1), (8, 8, 1), (4, 4, 1), (16, 4, 1), (32, 2, 1), (4, 1, 1)]
SWEEP_SP = {2: (3, 2, 5), 4: (2, 3, 5)}


def up(id_, ci, co, k, S, sp, pad, n=2, layout=None, bias=True, dbias=True, nums=None):
    return UpRow(id_, ci, co, tuple(k), S, tuple(sp), tuple(pad), n, layout or {}, bias, dbias, nums or {})


def _axis_kernel(axis, taps, pad):
    k, p = [1, 1, 1], [0, 0, 0]
    k[axis], p[axis] = taps, pad
    return tuple(k), tuple(p)


# 6-tap kernels of the sweep: (kernel, padding) per (scale, position among the 6-tap instances): every axis at every scale, and the
# two kernels whose six taps span two axes
_SIX = {(2, 0): ((6, 1, 1), (2, 0, 0)), (2, 1): ((2, 3, 1), (1, 1, 0)), (2, 2): ((1, 3, 2), (0, 1, 1)),
        (4, 0): ((1, 6, 1), (0, 2, 0)), (4, 1): ((1, 1, 6), (0, 0, 3)), (4, 2): ((2, 3, 1), (0, 0, 0))}


def _sweep():
    rows = []
    for S in (2, 4):
        three = six = one = 0
        for ci, co, t in INSTANCES:
            if t == 3:
                axis = (three + (S == 4)) % 3
                pad = 0 if three == 1 else 2 if (three == 2 and S == 4) else 1          # 'same'; none; k - 1: taps wholly in the border
                k, p = _axis_kernel(axis, 3, pad)
                three += 1
            elif t == 6:
                k, p = _SIX[(S, six)]
                six += 1
            else:
                k, p = (1, 1, 1), ((1, 1, 1) if (one == 5 and S == 2) or (one == 1 and S == 4) else (0, 0, 0))   # padding on one tap: a border of bias
                one += 1
            rows.append(up("inst-ci%dco%dt%d-s%d-k%d%d%d-p%d%d%d" % ((ci, co, t, S) + k + p), ci, co, k, S, SWEEP_SP[S], p))
    return rows


UP_SWEEP = _sweep()

UP_CORNERS = [
    # 4104 slabs of 2 x 4 voxels: the forward's grid of 4096 makes a second trip of 8 slabs, the weight gradient's 1024 five trips
    up("fwd-slabs-over-grid", 4, 1, (1, 3, 1), 4, (513, 1, 1), (0, 0, 0),
       nums={"fwd": dict(hch=2, slabs=4104, grid=4096, gtrips=2, trips=1), "wgrad": dict(slabs=4104, grid=1024, gtrips=5, trips=1)}),
    # the same with slabs that are single rows of H (wo = 514: hch = 1, two slabs a plane, three lane trips): 2 x 1026 x 2 x 514 outputs
    up("fwd-slabs-over-grid-hch1", 4, 1, (3, 1, 1), 2, (513, 1, 257), (1, 0, 0),
       nums={"fwd": dict(hch=1, slabs=4104, grid=4096, gtrips=2, trips=3), "wgrad": dict(hch=1, slabs=4104, grid=1024, gtrips=5, trips=3),
             "dgrad": dict(rows=1026, passes=9)}),
    up("wo-over-1024", 4, 1, (3, 1, 1), 4, (1, 1, 257), (1, 0, 0),
       nums={"fwd": dict(hch=1, trips=5, slabs=32), "wgrad": dict(hch=1, trips=5), "dgrad": dict(per=4, passes=65)}),
    up("ragged-slab", 4, 1, (3, 1, 1), 2, (1, 3, 103), (1, 0, 0),
       nums={"fwd": dict(hch=4, slabs=8, trips=4), "wgrad": dict(hch=4, slabs=8, grid=8, trips=4)}),
    up("ragged-slab-s4", 8, 2, (1, 3, 1), 4, (1, 7, 10), (0, 1, 0), nums={"fwd": dict(hch=25, slabs=16, trips=4)}),
    up("dgrad-rows-over-grid-wc1", 4, 1, (3, 1, 1), 2, (66, 63, 1), (1, 0, 0),
       nums={"dgrad": dict(rows=8316, grid=8192, gtrips=2, per=32, passes=1)}),
    up("wc33-s2", 8, 1, (1, 1, 3), 2, (1, 1, 33), (0, 0, 1), nums={"dgrad": dict(per=32, passes=2)}),
    up("wc5-s4", 8, 1, (1, 1, 3), 4, (1, 1, 5), (0, 0, 1), nums={"dgrad": dict(per=4, passes=2)}),
    up("wc10-s4-three-passes", 4, 2, (1, 1, 3), 4, (1, 2, 10), (0, 0, 1), nums={"dgrad": dict(per=4, passes=3)}),
    up("wc70-s2-three-passes", 16, 1, (1, 3, 1), 2, (1, 2, 70), (0, 1, 0), nums={"dgrad": dict(per=32, passes=3)}),
    up("one-slab", 4, 1, (6, 1, 1), 4, (1, 1, 2), (1, 0, 0), n=1,
       nums={"fwd": dict(slabs=1, grid=1, gtrips=1), "wgrad": dict(slabs=1, grid=1)}),
    up("n3", 8, 1, (3, 1, 1), 4, (2, 2, 3), (1, 0, 0), n=3, nums={"dgrad": dict(rows=12)}),
]

UP_OPERANDS = [
    up("x-pitch-ci+4-from-ch4", 4, 2, (3, 1, 1), 2, (2, 3, 5), (1, 0, 0), layout={"x": (8, 4)}),
    up("x-pitch-ci+4-from-ch4-s4", 8, 1, (3, 1, 1), 4, (2, 2, 5), (1, 0, 0), layout={"x": (12, 4)}),
    up("y-pitch-co+1-from-ch1", 8, 1, (3, 1, 1), 4, (2, 2, 3), (1, 0, 0), layout={"y": (2, 1)}),
    up("y-pitch-co+3-from-ch1", 4, 4, (1, 1, 1), 2, (2, 3, 5), (0, 0, 0), layout={"y": (7, 1)}),
    up("x-and-y-pitched", 4, 2, (1, 3, 2), 2, (2, 3, 5), (0, 1, 1), layout={"x": (8, 4), "y": (3, 1)}),
    up("no-bias", 8, 2, (1, 3, 1), 2, (2, 3, 5), (0, 1, 0), bias=False),
    up("no-dbias", 4, 1, (1, 1, 3), 4, (2, 2, 3), (0, 0, 1), dbias=False),
]

UP_ROWS = UP_SWEEP + UP_CORNERS + UP_OPERANDS


def pair(id_, sp, s1=2, p1=2, k2=6, s2=2, p2=2, n=2, layout=None, dbias=True, nums=None):
    return PairRow(id_, n, tuple(sp), s1, p1, k2, s2, p2, layout or {}, dbias, nums or {})


PAIR_ROWS = [
    pair("k6s2p2-shipped-w65", (8, 9, 65), nums=dict(chunks=2, rows=72, grid=18, gtrips=1)),
    pair("k3s1p1-w63", (8, 9, 63), k2=3, s2=1, p2=1, nums=dict(chunks=1)),
    pair("k6s3p2-w64", (8, 9, 64), k2=6, s2=3, p2=2, nums=dict(chunks=1)),
    pair("k8s3p3-w130", (8, 9, 130), k2=8, s2=3, p2=3, nums=dict(chunks=3)),
    pair("k1s1p0-w1", (8, 9, 1), k2=1, s2=1, p2=0, nums=dict(chunks=1)),
    pair("k2s3p0-rows-without-a-tap", (8, 9, 5), k2=2, s2=3, p2=0),
    pair("k5s2p4", (8, 9, 7), k2=5, s2=2, p2=4),
    pair("k4s2p0", (8, 9, 3), k2=4, s2=2, p2=0),
    pair("first-s1p0", (8, 9, 6), s1=1, p1=0),
    pair("first-s3p5", (8, 9, 6), s1=3, p1=5),
    pair("first-s2p0-odd-d", (9, 9, 6), s1=2, p1=0),
    pair("rows-over-grid", (122, 69, 2), n=1, nums=dict(rows=4209, grid=1024, gtrips=2, chunks=1)),
    pair("rows-under-4", (2, 3, 4), n=1, nums=dict(rows=3, grid=1, gtrips=1)),
    pair("x-pitch-3-ch2", (8, 9, 5), layout={"x": (3, 2)}),
    pair("dy2-pitch-12-from-ch4", (8, 9, 5), layout={"dy2": (12, 4)}),
    pair("no-dbias1", (8, 9, 5), dbias=False),
]

UP_PAIRS = [(r, d) for r in UP_ROWS for d in DTYPES]
UP_IDS = ["%s-%s" % (r.id, d) for r, d in UP_PAIRS]
PAIR_PAIRS = [(r, d) for r in PAIR_ROWS for d in DTYPES]
PAIR_IDS = ["%s-%s" % (r.id, d) for r, d in PAIR_PAIRS]
