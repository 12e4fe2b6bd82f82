"""Augmentation kernels on one MI355X: `mri3d_warp3d` (affine, elastic, affine + elastic; image alone and
image + uint8 label in one pass) and `mri3d_bias_field_f32` on a batch of 2 x 160x192x160, timed with device events.
Achieved bytes/s count the algorithmic traffic only: every input read once plus every output written once.
    python tests/perf/augment_bench.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mri_epilepsy_diagnosis_amd.segmentation import transforms as T  # noqa: E402


def timed(fn, n=200, repeats=3):
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


S, shape = 2, (160, 192, 160)
nvox = S * int(np.prod(shape))
g = torch.Generator().manual_seed(0)
image = torch.randn((S,) + shape, generator=g).cuda()
label = (torch.rand((S,) + shape, generator=g) < 0.1).to(torch.uint8).cuda()
image_out, label_out = torch.empty_like(image), torch.empty_like(label)

rng = np.random.default_rng(0)
affine, elastic = T.RandomAffine(translation=2, seed=1), T.RandomElasticDeformation(seed=2)
A = np.stack([affine.plan(shape)[0][0].matrix[:3] for _ in range(S)])
grid = np.stack([elastic.plan(shape)[0][0].grid for _ in range(S)])
ident = np.broadcast_to(np.eye(4)[:3], (S, 3, 4))
# the parameters are uploaded once, ahead of the timed calls: a timed call is validation + one launch, nothing synchronous
A, grid, ident = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in (A, grid, ident))
cases = [("identity map, image", image, None, ident, None),
         ("affine, image", image, None, A, None),
         ("affine, image + u8 label", image, label, A, None),
         ("elastic, image", image, None, ident, grid),
         ("affine + elastic, image", image, None, A, grid),
         ("affine + elastic, image + u8 label", image, label, A, grid),
         ("affine, u8 label alone", None, label, A, None)]
for name, img, lab, a, gr in cases:
    nbytes = (8 * nvox if img is not None else 0) + (2 * nvox if lab is not None else 0)
    ms = timed(lambda: T.warp3d(img, lab, a, gr, 0.0, image_out=None if img is None else image_out,
                                label_out=None if lab is None else label_out))
    print("warp3d %-36s %.3f ms  %.2f TB/s  (%.1f Gvoxel/s)" % (name + ":", ms, nbytes / ms / 1e9, nvox / ms / 1e6))

for order in (0, 3):
    coef = rng.uniform(-0.5, 0.5, (S, T.n_coefficients(order)))
    scratch = image.clone()
    for name, src, dst in (("out of place", image, image_out), ("in place", scratch, scratch)):
        ms = timed(lambda: T.bias_field(src, coef, order, out=dst))
        print("bias_field order %d %-13s %.3f ms  %.2f TB/s" % (order, name + ":", ms, 8 * nvox / ms / 1e9))
