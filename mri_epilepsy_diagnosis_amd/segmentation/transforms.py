"""Training augmentation on the device — SURVEY §8 row f5: the random stages of the reference's TorchIO pipeline.

Reference call site (segmentation/results_validation.ipynb, the `training_transform` cell; pretraining_3d_unet.ipynb cell 24;
applied through `torchio.ImagesDataset(subjects, transform=transform)`, segmentation/routine.py:91):

    Compose([HistogramStandardization(landmarks_dict={MRI: landmarks}), RandomBiasField(),
             ZNormalization(masking_method=ZNormalization.mean), CropOrPad((192, 192, 192)), RandomFlip(axes=(0,)),
             OneOf({RandomAffine(): 0.8, RandomElasticDeformation(): 0.2})])

The classes below carry TorchIO's names and arguments so that list can be written verbatim; they act on the subject dicts of
`patches.py`, {MRI: {DATA: (1,D,H,W)}, LABEL: {DATA: (1,D,H,W)}}, on the device.  TorchIO itself is absent from the reference
tree: the arithmetic is this project's definition (include/mri3d.h, "Augmentation"; float64 restatement in
tests/augment_ref.py) — "parity unpinned", like the patch pipeline.

The reference's lists open with two more lines, commented out: `RescaleIntensity((0, 1)),  # so that there are no negative values
for RandomMotion` and `RandomMotion()`; segmentation/routine.py imports both names.  Both are here, under the same terms (TorchIO
absent, "parity unpinned"; float64 restatement in tests/motion_ref.py).  RandomMotion needs no Fourier transform: TorchIO fills
slabs of the shifted spectrum along the LAST axis only, so the transforms along the other two axes cancel and the artefact is a
sum of 1-D circular filters along w over the unmoved volume and its K moved copies (`motion_coefficients`, `kspace_mix`;
derivation in include/mri3d.h).

Every random number is drawn on the HOST with numpy's `default_rng` (as `patches.Queue` does): which parameters are drawn is a
property of the seed, not of TorchIO.  A transform first PLANS — draws its parameters for a volume shape and records them in
`last_params` — and then the plan runs: flips, affines and an elastic deformation that are adjacent in a `Compose` fold into ONE
`mri3d_warp3d` launch (a flip is an affine with -1 on the diagonal), so the image is interpolated once and image and label share
the pass.  A container hands its generator to its children: inside `Compose(..., seed=s)` or a `Queue`, `s` decides everything.
There is no CPU path: every transform raises on a CPU tensor.
"""
import copy
import ctypes

import numpy as np
import torch

from .. import _lib
from ..classification import preprocessing
from ..ops import _ptr, _stream
from .patches import DATA, LABEL, MRI  # noqa: F401  (MRI re-exported for `landmarks_dict={MRI: ...}`)

LABEL_DTYPES = (torch.uint8, torch.int16, torch.int32, torch.float32)


# ------------------------------------------------------------------ device ops
def _require_cuda(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s: needs a ROCm device tensor (got %s); there is no CPU fallback"
                           % (what, getattr(t, "device", type(t))))


def _upload(a, device):
    """fp32 device copy of a host array; a float32 device tensor (parameters uploaded ahead of time) is used as it is."""
    if isinstance(a, torch.Tensor):
        _require_cuda(a, "warp3d")
        return a.to(torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def warp3d(image=None, label=None, affine=None, grid=None, pad=0.0, image_out=None, label_out=None):
    """One `mri3d_warp3d` launch over a batch.  image: (S,D,H,W) float32 or None; label: (S,D,H,W) uint8 / int16 / int32 /
    float32 (raw bits, nearest neighbour) or None; affine: (S,3,4) array (rounded to fp32 here, once); grid: (S,3,gd,gh,gw)
    control points or None (both may also be float32 device tensors uploaded earlier); pad: a number, or a device tensor of
    S floats.  Returns (image_out, label_out)."""
    first = image if image is not None else label
    if first is None:
        raise ValueError("warp3d: neither an image nor a label map given")
    for t in (image, label, image_out, label_out):
        if t is not None:
            _require_cuda(t, "warp3d")
    if image is not None and image.dtype != torch.float32:
        raise RuntimeError("warp3d: the image must be float32, got %s" % image.dtype)
    if label is not None and label.dtype not in LABEL_DTYPES:
        raise RuntimeError("warp3d: label maps may be uint8, int16, int32 or float32, got %s" % label.dtype)
    if first.dim() != 4 or (image is not None and label is not None and image.shape != label.shape):
        raise ValueError("warp3d: image and label must be (S, D, H, W) of one shape")
    s, d, h, w = (int(v) for v in first.shape)
    A = affine if isinstance(affine, torch.Tensor) else np.asarray(affine, dtype=np.float64).reshape(-1, 3, 4)
    if tuple(A.shape) != (s, 3, 4):
        raise ValueError("warp3d: affine maps %s for %d subjects, expected (S, 3, 4)" % (tuple(A.shape), s))
    dev = first.device
    image = None if image is None else image.contiguous()
    label = None if label is None else label.contiguous()
    if image is not None and image_out is None:
        image_out = torch.empty_like(image)
    if label is not None and label_out is None:
        label_out = torch.empty_like(label)
    A_dev = _upload(A, dev)
    gd = gh = gw = 0
    g_dev = None
    if grid is not None:
        grid = grid if isinstance(grid, torch.Tensor) else np.asarray(grid)
        if grid.ndim != 5 or tuple(grid.shape[:2]) != (s, 3):
            raise ValueError("warp3d: the control grid must be (S, 3, gd, gh, gw), got %s" % (grid.shape,))
        gd, gh, gw = (int(v) for v in grid.shape[2:])
        g_dev = _upload(grid, dev)
    pad_dev = None
    if isinstance(pad, torch.Tensor):
        _require_cuda(pad, "warp3d")
        pad_dev = pad.to(torch.float32).contiguous().view(-1)
        if pad_dev.numel() != s:
            raise ValueError("warp3d: %d pad values for %d subjects" % (pad_dev.numel(), s))
        pad = 0.0
    L = _lib.lib()
    _lib.check(L.mri3d_warp3d(_ptr(image), _ptr(image_out), _ptr(label), _ptr(label_out),
                              0 if label is None else label.element_size(), s, d, h, w, _ptr(A_dev), _ptr(g_dev), gd, gh, gw,
                              float(pad), _ptr(pad_dev), _stream()), "warp3d")
    return image_out, label_out


def bias_field(x, coefficients, order, out=None):
    """y = x * exp(P) over a batch (S,D,H,W) of float32 volumes; coefficients: (S, ncoef(order)) host array.  `out` may be `x`."""
    _require_cuda(x, "bias_field")
    if out is not None:
        _require_cuda(out, "bias_field")
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("bias_field: needs a float32 (S, D, H, W) tensor, got %s %s" % (x.dtype, tuple(x.shape)))
    x = x.contiguous()
    s, d, h, w = (int(v) for v in x.shape)
    c = np.ascontiguousarray(coefficients, dtype=np.float32).reshape(s, -1)
    order = int(order)
    if order >= 0 and c.shape[1] != n_coefficients(order):
        raise ValueError("bias_field: order %d takes %d coefficients per subject, got %d" % (order, n_coefficients(order), c.shape[1]))
    if out is None:
        out = torch.empty_like(x)
    L = _lib.lib()
    _lib.check(L.mri3d_bias_field_f32(_ptr(x), _ptr(out), s, d, h, w, c.ctypes.data_as(ctypes.c_void_p), order, _stream()),
               "bias_field")
    return out


def n_coefficients(order):
    return (order + 1) * (order + 2) * (order + 3) // 6


def kspace_mix(images, coef, out=None):
    """One `mri3d_kspace_mix_f32` launch: out[i,d,h,z] = sum_m sum_z' coef[i,m,(z - z') mod W] images[i,m,d,h,z'].
    images: (S,n,D,H,W) float32 device tensor; coef: (S,n,W) host array (rounded to fp32 here, once) or float32 device tensor;
    out: (S,D,H,W) float32 device tensor that overlaps neither.  Returns out."""
    _require_cuda(images, "kspace_mix")
    if out is not None:
        _require_cuda(out, "kspace_mix")
    if images.dtype != torch.float32 or images.dim() != 5:
        raise RuntimeError("kspace_mix: needs a float32 (S, n, D, H, W) tensor, got %s %s" % (images.dtype, tuple(images.shape)))
    images = images.contiguous()
    s, n, d, h, w = (int(v) for v in images.shape)
    if isinstance(coef, torch.Tensor):
        _require_cuda(coef, "kspace_mix")
        c_dev = coef.to(torch.float32).contiguous()
    else:
        c_dev = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float32)).to(images.device)
    if tuple(c_dev.shape) != (s, n, w):
        raise ValueError("kspace_mix: coefficients %s for images %s, expected (S, n, W)" % (tuple(c_dev.shape), tuple(images.shape)))
    if out is None:
        out = torch.empty((s, d, h, w), dtype=torch.float32, device=images.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (s, d, h, w) or not out.is_contiguous():
        raise ValueError("kspace_mix: out must be a contiguous float32 %s tensor" % ((s, d, h, w),))
    L = _lib.lib()
    _lib.check(L.mri3d_kspace_mix_f32(_ptr(images), _ptr(out), s, n, d, h, w, _ptr(c_dev), _stream()), "kspace_mix")
    return out


def motion_coefficients(times, w, n):
    """The 1-D filters of a motion artefact, float64: (coef (n, w), slabs).  TorchIO's rule, restated: with K = n - 1 ascending
    `times`, the slab ends are e_k = floor(w times[k]), then w; slab j covers the shifted-spectrum positions [e_{j-1}, e_j)
    along the last axis (empty slabs are allowed) and is filled from list entry j, the list being the images (0 = unmoved,
    k = moved by transform k) with entries 0 and idx swapped first, idx = the smallest index with times[idx] > 0.5, or K if
    there is none.  Shifted position p holds frequency fftshift(arange(w))[p].  coef[m, r] = (1/w) sum_{k in S_m} cos(2 pi k r / w)
    over the frequencies S_m filled from image m; slabs = [(image, ini, fin), ...]."""
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    w, n = int(w), int(n)
    K = n - 1
    if w < 1 or n < 1 or len(times) != K or np.any(np.diff(times) < 0):
        raise ValueError("motion_coefficients: %d images take %d ascending times (got %r), w >= 1" % (n, K, times))
    order = list(range(n))
    above = np.nonzero(times > 0.5)[0]
    idx = int(above.min()) if len(above) else K
    order[0], order[idx] = order[idx], order[0]
    ends = [min(max(int(np.floor(w * t)), 0), w) for t in times] + [w]
    freq = np.fft.fftshift(np.arange(w))
    r = np.arange(w)
    coef = np.zeros((n, w), dtype=np.float64)
    slabs, ini = [], 0
    for j, fin in enumerate(ends):
        slabs.append((order[j], ini, fin))
        k = freq[ini:fin]
        # the angle's integer part is taken off exactly: cos(2 pi ((k r) mod w) / w)
        coef[order[j]] += np.cos(2.0 * np.pi * ((k[:, None] * r[None, :]) % w) / w).sum(axis=0) / w
        ini = max(ini, fin)
    return coef, slabs


# ------------------------------------------------------------------ plan steps (host descriptors)
class Warp:
    """s = M o + u(o): M a 4x4 homogeneous float64 matrix (output voxel -> source voxel), grid (3,gd,gh,gw) float64 or None,
    pad 'minimum' | number | None (None: the map never leaves the volume, e.g. a flip)."""
    kind = "warp"

    def __init__(self, matrix, grid=None, pad=None):
        self.matrix, self.grid, self.pad = np.asarray(matrix, dtype=np.float64), grid, pad

    def params(self):
        return {"matrix": self.matrix[:3].copy(), "grid": None if self.grid is None else self.grid.copy(), "pad": self.pad}


class Bias:
    kind = "bias"

    def __init__(self, coefficients, order):
        self.coefficients, self.order = coefficients, order


class Motion:
    """A motion artefact: K 4x4 float64 matrices (output voxel -> source voxel of moved copy k), the pad rule of the copies
    and the (K + 1, W) float64 filters of `motion_coefficients`.  K = 0 (a skipped transform) runs nothing.  `fold` never merges
    it with a neighbour: a warp before it and a warp after it stay two launches."""
    kind = "motion"

    def __init__(self, matrices=(), coef=None, pad="minimum"):
        self.matrices = np.asarray(matrices, dtype=np.float64).reshape(-1, 4, 4)
        self.coef, self.pad = coef, pad


class Call:
    """A deterministic stage: fn(images, labels) -> (images, labels) on dicts of (S,D,H,W) device tensors."""
    kind = "call"

    def __init__(self, fn):
        self.fn = fn


def fold(steps):
    """Merge adjacent Warp steps.  Stages run in list order, so the folded map is the composition s_1(s_2(...(o))): a run of
    affine maps multiplies up (M = M_1 M_2 ...), and an elastic stage closes the run — its displacement, drawn in its own
    input frame, is carried into the source frame by the linear part of what precedes it:
    M_1 (M_2 o + u(o)) = M_1 M_2 o + L_1 u(o).  Whatever follows an elastic stage starts a new run."""
    out = []
    for st in steps:
        prev = out[-1] if out else None
        if st.kind == "warp" and prev is not None and prev.kind == "warp" and prev.grid is None:
            grid = None if st.grid is None else np.einsum("ab,bdhw->adhw", prev.matrix[:3, :3], st.grid)
            out[-1] = Warp(prev.matrix @ st.matrix, grid, st.pad if st.pad is not None else prev.pad)
        else:
            out.append(st)
    return out


def _identity_like(step):
    return Warp(np.eye(4)) if step.kind == "warp" else step


def _minimum(x):
    """(S,) device tensor of per-subject minima: `order_statistics(x, [0])` per subject, as RandomAffine's 'minimum' is
    specified.  The result stays on the device and goes to the kernel as `pad_values` (it is `percentile`, not
    `order_statistics`, that brings values to the host)."""
    return torch.cat([preprocessing.order_statistics(x[i], [0]) for i in range(x.shape[0])])


def _run_warp(images, labels, steps):
    A = np.stack([st.matrix[:3] for st in steps])
    shapes = {st.grid.shape for st in steps if st.grid is not None}
    if len(shapes) > 1:
        raise ValueError("one control-grid shape per launch, got %s" % sorted(shapes))
    grid = None
    if shapes:
        zero = np.zeros(next(iter(shapes)))
        grid = np.stack([zero if st.grid is None else st.grid for st in steps])
    # one launch takes one image and one label map: the k-th image rides with the k-th label (the usual subject has one of
    # each, so one launch), further entries get launches of their own under the same map
    names_i, names_l = list(images), list(labels)
    for k in range(max(len(names_i), len(names_l))):
        img = images[names_i[k]] if k < len(names_i) else None
        lab = labels[names_l[k]] if k < len(names_l) else None
        pad = 0.0
        if img is not None:
            pads = [st.pad for st in steps]
            if any(p == "minimum" for p in pads):
                pad = _minimum(img)
                for i, p in enumerate(pads):
                    if p != "minimum":
                        pad[i] = float(p or 0.0)
            elif len(set(pads)) == 1:
                pad = float(pads[0] or 0.0)
            else:
                pad = torch.tensor([float(p or 0.0) for p in pads], dtype=torch.float32, device=img.device)
        o_img, o_lab = warp3d(img, lab, A, grid, pad)
        if img is not None:
            images[names_i[k]] = o_img
        if lab is not None:
            labels[names_l[k]] = o_lab
    return images, labels


def _run_motion(images, steps):
    """The K moved copies of every subject by the existing `warp3d` (image only, the step's pad rule) into an (S, K + 1, D, H, W)
    buffer whose slot 0 is the input, then ONE `kspace_mix` launch for the batch.  Label maps are not touched."""
    K = len(steps[0].matrices)
    if K == 0:
        return images
    coef = np.stack([st.coef for st in steps])
    out = {}
    for name, img in images.items():
        s = int(img.shape[0])
        buf = torch.empty((s, K + 1) + tuple(img.shape[1:]), dtype=torch.float32, device=img.device)
        buf[:, 0].copy_(img)
        minimum = _minimum(img) if any(st.pad == "minimum" for st in steps) else None
        # a launch writes contiguous volumes, and slot k of subject i is one: a launch per (subject, copy)
        for i, st in enumerate(steps):
            pad = minimum[i:i + 1] if st.pad == "minimum" else float(st.pad or 0.0)
            for k in range(K):
                warp3d(img[i:i + 1], None, st.matrices[k, :3][None], None, pad, image_out=buf[i, k + 1][None])
        out[name] = kspace_mix(buf, coef)
    return out


def execute(images, labels, plans):
    """Run per-subject plans on a batch: images / labels are dicts name -> (S,D,H,W) device tensors, plans S folded step lists.
    When all plans have the same step kinds, every warp and bias step is ONE launch for the batch; otherwise each subject runs
    on its own.  Motion steps count as the same kind only with the same number of moved copies."""
    kinds = [tuple(st.kind if st.kind != "motion" else ("motion", len(st.matrices)) for st in p) for p in plans]
    if len(set(kinds)) > 1:
        parts = [execute({k: v[i:i + 1] for k, v in images.items()}, {k: v[i:i + 1] for k, v in labels.items()}, [plans[i]])
                 for i in range(len(plans))]
        return ({k: torch.cat([p[0][k] for p in parts]) for k in images}, {k: torch.cat([p[1][k] for p in parts]) for k in labels})
    images, labels = dict(images), dict(labels)
    for j, kind in enumerate(kinds[0]):
        steps = [p[j] for p in plans]
        if kind == "warp":
            images, labels = _run_warp(images, labels, steps)
        elif kind == "bias":
            orders = {st.order for st in steps}
            if len(orders) > 1:
                raise ValueError("one bias-field order per launch")
            coef = np.stack([st.coefficients for st in steps])
            images = {k: bias_field(v, coef, steps[0].order) for k, v in images.items()}
        elif kind == "call":
            outs = [st.fn({k: v[i:i + 1] for k, v in images.items()}, {k: v[i:i + 1] for k, v in labels.items()})
                    for i, st in enumerate(steps)]
            images = {k: torch.cat([o[0][k] for o in outs]) for k in images}
            labels = {k: torch.cat([o[1][k] for o in outs]) for k in labels}
        else:
            images = _run_motion(images, steps)
    return images, labels


def split_subject(subject, what):
    """(images, labels, shape) of a subject dict: the LABEL entry is a label map, every other entry with DATA an intensity image."""
    images, labels = {}, {}
    for k, v in subject.items():
        if isinstance(v, dict) and DATA in v:
            t = v[DATA]
            _require_cuda(t, what)
            if t.dim() != 4 or t.shape[0] != 1:
                raise ValueError("%s: images must be (1, D, H, W), got %s" % (what, tuple(t.shape)))
            (labels if k == LABEL else images)[k] = t
    if not images and not labels:
        raise ValueError("%s: the subject holds no image" % what)
    shape = tuple(int(v) for v in next(iter({**images, **labels}.values())).shape[1:])
    return images, labels, shape


# ------------------------------------------------------------------ transforms
class Transform:
    """Base: `p` = probability of applying the transform, `seed` = an int or a numpy Generator for stand-alone use."""

    def __init__(self, p=1, seed=None):
        self.p = float(p)
        self.rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
        self.last_params = None

    def plan(self, shape, rng=None):
        """Draw this call's parameters for a (D, H, W) volume on the host.  Returns (steps, shape after the transform)."""
        rng = self.rng if rng is None else rng
        shape = tuple(int(v) for v in shape)
        if self.p < 1 and rng.random() >= self.p:
            self.last_params = {"applied": False}
            return [_identity_like(st) for st in self._skeleton(shape)], shape
        return self._plan(shape, rng)

    def _skeleton(self, shape):
        """The steps a skipped transform leaves behind (identity warps keep batched plans in lockstep)."""
        return []

    def _plan(self, shape, rng):
        raise NotImplementedError

    def __call__(self, subject):
        images, labels, shape = split_subject(subject, type(self).__name__)
        steps, _ = self.plan(shape)
        images, labels = execute(images, labels, [fold(steps)])
        out = dict(subject)
        for k, v in {**images, **labels}.items():
            out[k] = dict(subject[k])
            out[k][DATA] = v
        return out


def _pair(v, name, symmetric=True):
    if isinstance(v, (int, float, np.integer, np.floating)):
        if v < 0:
            raise ValueError("%s must not be negative" % name)
        return (-float(v), float(v)) if symmetric else (float(v), float(v))
    v = tuple(float(x) for x in v)
    if len(v) != 2 or v[0] > v[1]:
        raise ValueError("%s must be a number or an ascending (min, max) pair" % name)
    return v


def flip_matrix(flipped, shape):
    """4x4 map of a flip: o -> (N - 1) - o on the flipped axes (a -1 on the diagonal)."""
    M = np.eye(4)
    for a, n in enumerate(shape):
        if flipped[a]:
            M[a, a], M[a, 3] = -1.0, float(n - 1)
    return M


def _rotation(axis, degrees):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    i, j = [a for a in range(3) if a != axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def affine_matrix(scales, degrees, translation, shape):
    """4x4 float64 map output voxel -> source voxel: s = c + R diag(1 / scales) (o - c) + t with c = (N - 1) / 2, the centre
    folded into the offset column.  A scale above 1 magnifies the content; R = R_0 R_1 R_2, R_k a rotation about stored axis k."""
    L = _rotation(0, degrees[0]) @ _rotation(1, degrees[1]) @ _rotation(2, degrees[2]) @ np.diag(1.0 / np.asarray(scales, dtype=np.float64))
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    M = np.eye(4)
    M[:3, :3] = L
    M[:3, 3] = c - L @ c + np.asarray(translation, dtype=np.float64)
    return M


class RandomFlip(Transform):
    """torchio.RandomFlip(axes=(0,), flip_probability=0.5): axis 0 is the first spatial axis of the stored tensor."""

    def __init__(self, axes=(0,), flip_probability=0.5, p=1, seed=None):
        super().__init__(p, seed)
        self.axes = (int(axes),) if isinstance(axes, (int, np.integer)) else tuple(int(a) for a in axes)
        if any(a not in (0, 1, 2) for a in self.axes):
            raise ValueError("RandomFlip: axes must be among 0, 1, 2, got %r" % (axes,))
        self.flip_probability = float(flip_probability)

    def _skeleton(self, shape):
        return [Warp(np.eye(4))]

    def _plan(self, shape, rng):
        flipped = [False, False, False]
        for a in self.axes:
            flipped[a] = bool(rng.random() < self.flip_probability)
        M = flip_matrix(flipped, shape)
        self.last_params = {"applied": True, "flipped": tuple(flipped), "matrix": M[:3].copy()}
        return [Warp(M)], shape


class RandomAffine(Transform):
    """torchio.RandomAffine(scales=(0.9, 1.1), degrees=10, isotropic=False, translation=0, default_pad_value='minimum'):
    per-axis scale, rotation (degrees) and translation (voxels) uniform in their ranges, about the volume centre (N - 1) / 2;
    trilinear for the image, nearest for the label.  'minimum' is the image's minimum, from `order_statistics(x, [0])`."""

    def __init__(self, scales=(0.9, 1.1), degrees=10, isotropic=False, translation=0, default_pad_value="minimum", p=1, seed=None):
        super().__init__(p, seed)
        self.scales = _pair(scales, "scales", symmetric=False)
        if self.scales[0] <= 0:
            raise ValueError("RandomAffine: scales must be positive")
        self.degrees, self.translation = _pair(degrees, "degrees"), _pair(translation, "translation")
        self.isotropic = bool(isotropic)
        if default_pad_value != "minimum" and not isinstance(default_pad_value, (int, float)):
            raise ValueError("RandomAffine: default_pad_value is 'minimum' or a number (Otsu padding is out of scope)")
        self.default_pad_value = default_pad_value

    def _skeleton(self, shape):
        return [Warp(np.eye(4))]

    def _plan(self, shape, rng):
        scales = rng.uniform(*self.scales, size=3)
        if self.isotropic:
            scales[:] = scales[0]
        degrees = rng.uniform(*self.degrees, size=3)
        translation = rng.uniform(*self.translation, size=3)
        M = affine_matrix(scales, degrees, translation, shape)
        self.last_params = {"applied": True, "scales": scales, "degrees": degrees, "translation": translation, "matrix": M[:3].copy()}
        return [Warp(M, None, self.default_pad_value)], shape


def _triple(v, cast):
    if isinstance(v, (int, float, np.integer, np.floating)):
        return cast(v), cast(v), cast(v)
    v = tuple(cast(x) for x in v)
    if len(v) != 3:
        raise ValueError("expected 3 values, got %r" % (v,))
    return v


class RandomElasticDeformation(Transform):
    """torchio.RandomElasticDeformation(num_control_points=7, max_displacement=7.5, locked_borders=2): a cubic B-spline
    displacement field whose control points are uniform in +-max_displacement voxels, the outer `locked_borders` layers zero.
    The image is padded with its minimum where the deformed grid leaves it."""

    def __init__(self, num_control_points=7, max_displacement=7.5, locked_borders=2, p=1, seed=None):
        super().__init__(p, seed)
        self.num_control_points = _triple(num_control_points, int)
        self.max_displacement = _triple(max_displacement, float)
        self.locked_borders = int(locked_borders)
        if min(self.num_control_points) < 4:
            raise ValueError("RandomElasticDeformation: at least 4 control points per axis")
        if self.locked_borders not in (0, 1, 2) or min(self.max_displacement) < 0:
            raise ValueError("RandomElasticDeformation: locked_borders in 0..2, max_displacement >= 0")

    def _skeleton(self, shape):
        return [Warp(np.eye(4))]

    def _plan(self, shape, rng):
        g = self.num_control_points
        grid = rng.uniform(-1.0, 1.0, size=(3,) + g) * np.asarray(self.max_displacement)[:, None, None, None]
        b = self.locked_borders
        if b:
            for axis in (1, 2, 3):
                sl = [slice(None)] * 4
                for edge in (slice(0, b), slice(g[axis - 1] - b, None)):
                    sl[axis] = edge
                    grid[tuple(sl)] = 0.0
        self.last_params = {"applied": True, "grid": grid.copy()}
        return [Warp(np.eye(4), grid, "minimum")], shape


class RandomBiasField(Transform):
    """torchio.RandomBiasField(coefficients=0.5, order=3): y = x exp(P), P a polynomial of the given order in the voxel
    position mapped to [-1, 1]^3, its coefficients uniform in +-`coefficients` (a (min, max) pair is accepted)."""

    def __init__(self, coefficients=0.5, order=3, p=1, seed=None):
        super().__init__(p, seed)
        self.coefficients = _pair(coefficients, "coefficients")
        self.order = int(order)
        if not 0 <= self.order <= 3:
            raise ValueError("RandomBiasField: order 0..3 (the kernel's limit), got %d" % self.order)

    def _skeleton(self, shape):
        return [Bias(np.zeros(n_coefficients(self.order), np.float32), self.order)]

    def _plan(self, shape, rng):
        coef = rng.uniform(*self.coefficients, size=n_coefficients(self.order)).astype(np.float32)
        self.last_params = {"applied": True, "coefficients": coef.copy(), "order": self.order}
        return [Bias(coef, self.order)], shape


class RandomMotion(Transform):
    """torchio.RandomMotion(degrees=10, translation=10, num_transforms=2): the volume is moved rigidly `num_transforms` = K
    times — three angles uniform in +-degrees, three translations uniform in +-translation voxels (the project's unit-spacing
    convention; (min, max) pairs are accepted), about the volume centre, trilinear, padded with the image minimum — and the
    K + 1 spectra are spliced along the last axis at the times t_k = k/(K+1) + U(-0.3/(K+1), +0.3/(K+1)), k = 1..K
    (`motion_coefficients`).  Image only: label maps pass through with the same bits, no launch and no copy.  TorchIO is
    absent from the reference tree: this is the project's restatement, "parity unpinned".
    `last_params`: times, degrees (K,3), translation (K,3), matrices (K,3,4) float64 before the fp32 rounding, slabs, coefficients."""

    def __init__(self, degrees=10, translation=10, num_transforms=2, p=1, seed=None):
        super().__init__(p, seed)
        self.degrees, self.translation = _pair(degrees, "degrees"), _pair(translation, "translation")
        self.num_transforms = int(num_transforms)
        if not 1 <= self.num_transforms <= 7:
            raise ValueError("RandomMotion: num_transforms 1..7 (the kernel mixes at most 8 volumes), got %d" % self.num_transforms)

    def _skeleton(self, shape):
        return [Motion()]

    def _plan(self, shape, rng):
        K = self.num_transforms
        degrees, translation = np.empty((K, 3)), np.empty((K, 3))
        for k in range(K):
            degrees[k] = rng.uniform(*self.degrees, size=3)
            translation[k] = rng.uniform(*self.translation, size=3)
        step = 1.0 / (K + 1)
        times = step * np.arange(1, K + 1) + rng.uniform(-0.3 * step, 0.3 * step, size=K)
        matrices = np.stack([affine_matrix((1.0, 1.0, 1.0), degrees[k], translation[k], shape) for k in range(K)])
        coef, slabs = motion_coefficients(times, shape[2], K + 1)
        self.last_params = {"applied": True, "times": times, "degrees": degrees, "translation": translation,
                            "matrices": matrices[:, :3].copy(), "slabs": slabs, "coefficients": coef.copy()}
        return [Motion(matrices, coef, "minimum")], shape


class Compose(Transform):
    """torchio.Compose([...]): the stages in order, adjacent spatial stages folded into one resampling (see `fold`).
    `last_params` = {'stages': each stage's own record, 'warps': the folded maps as launched (float64, before the fp32 rounding)}."""

    def __init__(self, transforms, p=1, seed=None):
        super().__init__(p, seed)
        self.transforms = list(transforms)

    def _plan(self, shape, rng):
        steps = []
        for t in self.transforms:
            more, shape = t.plan(shape, rng)
            steps += more
        steps = fold(steps)
        self.last_params = {"applied": True, "stages": [copy.deepcopy(t.last_params) for t in self.transforms],
                            "warps": [st.params() for st in steps if st.kind == "warp"]}
        return steps, shape


class OneOf(Transform):
    """torchio.OneOf({transform: weight, ...}): one of the transforms, chosen with probability proportional to its weight."""

    def __init__(self, transforms, p=1, seed=None):
        super().__init__(p, seed)
        if not isinstance(transforms, dict):
            transforms = {t: 1.0 for t in transforms}
        self.transforms = list(transforms)
        w = np.asarray([float(transforms[t]) for t in self.transforms], dtype=np.float64)
        if len(w) == 0 or np.any(w < 0) or w.sum() <= 0:
            raise ValueError("OneOf: weights must be non-negative and not all zero")
        self.probabilities = w / w.sum()

    def _skeleton(self, shape):
        return self.transforms[0]._skeleton(shape)

    def _plan(self, shape, rng):
        choice = int(rng.choice(len(self.transforms), p=self.probabilities))
        steps, shape = self.transforms[choice].plan(shape, rng)
        self.last_params = {"applied": True, "choice": choice, "params": copy.deepcopy(self.transforms[choice].last_params)}
        return steps, shape


# ------------------------------------------------------------------ the deterministic stages, over the existing device functions
class HistogramStandardization(Transform):
    """torchio.HistogramStandardization(landmarks_dict={MRI: landmarks}) over `preprocessing.normalize`."""

    def __init__(self, landmarks_dict, p=1, seed=None):
        super().__init__(p, seed)
        self.landmarks_dict = {k: np.asarray(v) for k, v in landmarks_dict.items()}

    @classmethod
    def train(cls, images, image_key=None, cutoff=None, mask=None, masking_function=None, output_path=None):
        """torchio.HistogramStandardization.train over `preprocessing.train_landmarks`, with volumes that are already on the device
        where TorchIO takes paths: `images` is a sequence of device tensors, or of subject dicts whose `image_key` entry is one.
        Returns the landmark vector, so that HistogramStandardization(landmarks_dict={MRI: HistogramStandardization.train(...)})
        reads like the reference's notebook."""
        images = list(images)
        if any(isinstance(s, dict) for s in images):
            if image_key is None:
                raise ValueError("HistogramStandardization.train: subject dicts need image_key")
            images = [s[image_key] for s in images]
        return preprocessing.train_landmarks(images, cutoff=cutoff, mask=mask, masking_function=masking_function,
                                             output_path=output_path)

    def _fn(self, images, labels):
        return {k: (preprocessing.normalize(v, self.landmarks_dict[k]) if k in self.landmarks_dict else v)
                for k, v in images.items()}, labels

    def _skeleton(self, shape):
        return [Call(lambda images, labels: (images, labels))]

    def _plan(self, shape, rng):
        self.last_params = {"applied": True}
        return [Call(self._fn)], shape


class RescaleIntensity(Transform):
    """torchio.RescaleIntensity(out_min_max, percentiles=(0, 100)) over `preprocessing.percentile` and
    `mri3d_piecewise_linear_f32`: the cut-offs are the two percentiles of the whole image; values are clipped to them and
    mapped linearly onto out_min_max.  An image without range (equal cut-offs) maps to out_min.  Labels are untouched.
    TorchIO is absent from the reference tree: "parity unpinned".  The cut-offs are known when the stage RUNS: this
    instance's `last_params['cutoffs']` = {image name: (low, high)} float64 is filled in then (a `Compose` copies its stages'
    records at planning time, before that)."""

    def __init__(self, out_min_max, percentiles=(0, 100), p=1, seed=None):
        super().__init__(p, seed)
        self.out_min_max = _pair(out_min_max, "out_min_max", symmetric=False)
        self.percentiles = _pair(percentiles, "percentiles", symmetric=False)
        if not 0 <= self.percentiles[0] <= self.percentiles[1] <= 100:
            raise ValueError("RescaleIntensity: percentiles must lie in 0..100, got %r" % (percentiles,))

    def _rescale(self, v):
        low, high = (float(c) for c in preprocessing.percentile(v, self.percentiles))
        out_min, out_max = self.out_min_max
        if high > low:
            slope = (out_max - out_min) / (high - low)
            edges = np.asarray([low, high], dtype=np.float64)
            slopes = np.asarray([0.0, slope, 0.0], dtype=np.float64)
            intercepts = np.asarray([out_min, out_min - slope * low, out_max], dtype=np.float64)
        else:
            edges, slopes, intercepts = np.zeros(0), np.zeros(1), np.asarray([out_min], dtype=np.float64)
        x = v.contiguous()
        y = torch.empty_like(x)
        as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None  # noqa: E731
        _lib.check(_lib.lib().mri3d_piecewise_linear_f32(_ptr(x), _ptr(y), x.numel(), as_p(edges), as_p(slopes), as_p(intercepts),
                                                         len(slopes), _stream()), "piecewise_linear")
        return y, (low, high)

    def _fn(self, images, labels):
        out, cutoffs = {}, {}
        for k, v in images.items():
            if v.dtype != torch.float32:
                raise RuntimeError("RescaleIntensity: images must be float32, got %s for %r" % (v.dtype, k))
            out[k], cutoffs[k] = self._rescale(v)
        self.last_params = {"applied": True, "cutoffs": cutoffs}
        return out, labels

    def _skeleton(self, shape):
        return [Call(lambda images, labels: (images, labels))]

    def _plan(self, shape, rng):
        self.last_params = {"applied": True, "cutoffs": {}}
        return [Call(self._fn)], shape


class ZNormalization(Transform):
    """torchio.ZNormalization(masking_method=ZNormalization.mean) over `preprocessing.z_normalize` (the only masking the
    reference uses, and the only one built)."""

    @staticmethod
    def mean(tensor):
        return tensor > tensor.mean()

    def __init__(self, masking_method=None, p=1, seed=None):
        super().__init__(p, seed)
        if masking_method is not ZNormalization.mean:
            raise NotImplementedError("ZNormalization: only masking_method=ZNormalization.mean is built")

    def _fn(self, images, labels):
        return {k: preprocessing.z_normalize(v)[0] for k, v in images.items()}, labels

    def _skeleton(self, shape):
        return [Call(lambda images, labels: (images, labels))]

    def _plan(self, shape, rng):
        self.last_params = {"applied": True}
        return [Call(self._fn)], shape


class CropOrPad(Transform):
    """torchio.CropOrPad(target_shape) over `preprocessing.crop_or_pad` (zero padding).  That kernel is float32-only: a label
    map of another dtype is refused here, not converted."""

    def __init__(self, target_shape, p=1, seed=None):
        super().__init__(p, seed)
        if self.p < 1:
            raise ValueError("CropOrPad changes the shape: p must be 1")
        self.target_shape = _triple(target_shape, int)

    def _fn(self, images, labels):
        for k, v in labels.items():
            if v.dtype != torch.float32:
                raise RuntimeError("CropOrPad: mri3d_crop_or_pad_f32 takes float32 volumes only; label map %r is %s — keep "
                                   "labels float32 up to here" % (k, v.dtype))
        cut = lambda v: preprocessing.crop_or_pad(v, self.target_shape)  # noqa: E731
        return {k: cut(v) for k, v in images.items()}, {k: cut(v) for k, v in labels.items()}

    def _plan(self, shape, rng):
        self.last_params = {"applied": True}
        return [Call(self._fn)], self.target_shape


class ImagesDataset:
    """torchio.ImagesDataset(subjects, transform=None) (segmentation/routine.py:91) for HBM-resident subject dicts."""

    def __init__(self, subjects, transform=None):
        self.subjects, self.transform = list(subjects), transform

    def __len__(self):
        return len(self.subjects)

    def __getitem__(self, index):
        subject = self.subjects[index]
        return subject if self.transform is None else self.transform(subject)
