"""Operator seam: one ``torch.autograd.Function`` per volumetric op, each a thin wrapper over the C-ABI HIP library.

Tensors keep torch's logical (N, C, D, H, W) shape but live in channels-last-3d memory (NDHWC), which is what the
kernels index.  Every op here requires a ROCm device tensor and the built ``libmri3d_hip.so``; there is no CPU or
eager-PyTorch fallback (a CPU tensor raises), so a green GPU test always means the HIP kernels ran.

Reference operators replaced (file:line in /root/reference):
  conv3d               nn.Conv3d            unet.UNet via segmentation/routine.py:346-356; AE_model.py:9-26; cnn_model.py:14
  conv3d_act           nn.Conv3d(1, 8|16, 3, padding=1) + PReLU/LeakyReLU/ReLU, the U-Net's first layer, as one operator
  conv_transpose3d     nn.ConvTranspose3d   AE_model.py:62-68,159
  norm_act             nn.BatchNorm3d / nn.InstanceNorm3d + PReLU/LeakyReLU/ReLU   AE_model.py:30-36; modified_3dunet.py:20-94
  max_pool3d           nn.MaxPool3d         AE_model.py:27; cnn_model.py:115-148,221
  upsample3d           nn.Upsample / F.interpolate   modified_3dunet.py:13; AE_model.py:70-73,119
  softmax_dice_loss    F.softmax + get_dice_loss + mean   segmentation/routine.py:239-253,272-274
  cat_channels / add   torch.cat(dim=1) / residual adds   modified_3dunet.py:108,158
  bayes_conv3d         BayesConv3d          3d_bayes_layers.py:195-232 (3d_bayes_unet.py::UNet3D(bayes=True))
  remap_labels         np.isin + boolean-mask writes of prepare_batch   segmentation/routine.py:185-196
  softmax_dice_index_loss   the same loss against a uint8 class map (2..32 classes)   segmentation/routine.py:272-274
  gaussian_kde / intensity_moments   scipy.stats.gaussian_kde over a volume's voxels   full_sample_classification.ipynb cell 9
Beyond the reference: mc_state / mc_accumulate / mc_finalize, the Monte-Carlo read-out of its stochastic models (no autograd);
confusion_counts / class_scores_from_confusion, per-class Dice and IoU of a multi-class mask; label_components / component_stats /
select_components, the connected components of a mask (scipy.ndimage.label's numbering), their tables and the masks they select;
softmax_ce_index_loss / softmax_dice_ce_index_loss, cross-entropy and focal loss against a class map, alone or fused with the index
Dice (the reference trains on Dice alone); edt_sq / edt_threshold / signed_sqdist / softmax_boundary_loss, the exact squared
Euclidean distance transform of a mask, ball morphology as its thresholds, the signed distance maps of a class map and the
boundary loss that reads them.
"""
import collections
import ctypes
import math

import torch

from . import _lib
from ._lib import (ACT_LEAKY, ACT_NONE, ACT_PRELU, ACT_RELU, BF16, F32, NORM_PASS_BWD, NORM_PASS_FWD, NORM_PASS_STATS, PASS_DGRAD,
                   PASS_FWD, PASS_WGRAD, UP_NEAREST, UP_TRILINEAR, ConvGeom, DiceGeom, NormGeom, NormPlanInfo, PoolGeom, UpGeom,
                   check)

CL3D = torch.channels_last_3d

# ----------------------------------------------------------------------------------------------- plumbing


def _require_device(*ts):
    """Activation tensors: float32 or bfloat16 on a ROCm device."""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "mri_epilepsy_diagnosis_amd ops run only on a ROCm device tensor (got %s); there is no CPU fallback"
                % t.device)
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("mri_epilepsy_diagnosis_amd ops: only float32 / bfloat16 tensors are supported, got %s"
                               % t.dtype)


def _require_param(*ts):
    """Parameters, statistics and targets: float32 on a ROCm device (bf16 regions keep fp32 master parameters)."""
    for t in ts:
        if t is None:
            continue
        _require_device(t)
        if t.dtype != torch.float32:
            raise RuntimeError("mri_epilepsy_diagnosis_amd ops: parameters must be float32, got %s" % t.dtype)


def _dt(t):
    return BF16 if t.dtype == torch.bfloat16 else F32


def _esz(t):
    return 2.0 if t.dtype == torch.bfloat16 else 4.0


# ----------------------------------------------------------------------------------------------- bf16 region
# BASELINE configs[3] ("3D U-Net bf16"): inside `with autocast():` every conv stores its output in bfloat16 (fp32
# accumulate), and all downstream volumetric ops follow the dtype of their input; parameters, statistics, parameter
# gradients and the loss stay fp32 (the reference itself is fp32-only, so the region is opt-in like torch.autocast).
_autocast_dtype = None


def autocast_dtype():
    """The storage dtype of the active `autocast` region, or None."""
    return _autocast_dtype


class autocast:
    def __init__(self, enabled=True, dtype=torch.bfloat16):
        if dtype is not torch.bfloat16:
            raise RuntimeError("mri_epilepsy_diagnosis_amd.autocast: only torch.bfloat16 is supported")
        self.new = dtype if enabled else None

    def __enter__(self):
        global _autocast_dtype
        self.prev = _autocast_dtype
        _autocast_dtype = self.new
        return self

    def __exit__(self, *exc):
        global _autocast_dtype
        _autocast_dtype = self.prev
        return False


def convert(x, dtype):
    """x.to(dtype) for NDHWC activations (fp32 <-> bf16, round-to-nearest-even) as a HIP pass; differentiable."""
    return _ConvertFn.apply(x, dtype)


def _convert_raw(x, dtype):
    L = _lib.lib()
    x, x_ld = _nd(x)
    n, c, d, h, w = x.shape
    y = torch.empty(x.shape, dtype=dtype, device=x.device, memory_format=CL3D)
    check(L.mri3d_convert_channels(_ptr(x), _dt(x), _ptr(y), _dt(y), n * d * h * w, c, x_ld, c, _stream()),
          "convert_channels")
    return y


class _ConvertFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        _require_device(x)
        ctx.src_dtype = x.dtype
        if x.dtype == dtype:
            return x.view_as(x)
        return _convert_raw(x, dtype)

    @staticmethod
    def backward(ctx, dy):
        if dy.dtype == ctx.src_dtype:
            return dy, None
        return _convert_raw(dy, ctx.src_dtype), None


def _is_ndhwc_dense(x):
    n, c, d, h, w = x.shape
    exp = (d * h * w * c, 1, h * w * c, w * c, c)
    for dim in range(5):
        if x.shape[dim] > 1 and x.stride(dim) != exp[dim]:
            return False
    return True


def _cl(x):
    """Return x with dense NDHWC memory (no copy if it already is)."""
    if x.dim() != 5:
        raise RuntimeError("expected a 5-D (N,C,D,H,W) tensor, got shape %s" % (tuple(x.shape),))
    if _is_ndhwc_dense(x):
        return x
    return x.contiguous(memory_format=CL3D)


def _pitch_of(x):
    """Voxel pitch ld if x's memory is NDHWC with pitch ld >= C (dense, or a channel slice of a wider NDHWC buffer),
    else None."""
    n, c, d, h, w = x.shape
    if c > 1 and x.stride(1) != 1:
        return None
    ld = None
    for size, stride, inner in ((w, x.stride(4), 1), (h, x.stride(3), w), (d, x.stride(2), h * w), (n, x.stride(0), d * h * w)):
        if size > 1:
            if stride % inner:
                return None
            cand = stride // inner
            if ld is None:
                ld = cand
            elif cand != ld:
                return None
    if ld is None:
        ld = c
    return ld if ld >= c else None


def _nd(x):
    """(tensor, ld): x itself when it is NDHWC with some voxel pitch (no copy), else a dense NDHWC copy."""
    if x.dim() != 5:
        raise RuntimeError("expected a 5-D (N,C,D,H,W) tensor, got shape %s" % (tuple(x.shape),))
    ld = _pitch_of(x)
    if ld is not None:
        return x, ld
    x = x.contiguous(memory_format=CL3D)
    return x, x.shape[1]


def _slice_view(buf, off, c):
    """Channel slice [off, off+c) of an NDHWC buffer as a logical (N, c, D, H, W) tensor (pitched view, no copy)."""
    return buf.narrow(1, off, c)


def _new(shape, like):
    return torch.empty(shape, dtype=like.dtype, device=like.device, memory_format=CL3D)


def _ptr(t, byte_offset=0):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_workspaces = {}


def _workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream); kernels using it are ordered on that stream."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def release_workspaces():
    """Drop the scratch buffers (explicit teardown; they are re-created on demand)."""
    _workspaces.clear()


class KernelTimer:
    """Optional per-operator device timing: when installed (bench.py), every C-ABI call made through `_timed` is
    bracketed by two events recorded on the stream the kernels are enqueued on (torch's current stream)."""

    MAX_LIVE = 512   # event pairs kept before they are folded into the totals (see fold())

    def __init__(self, only=None):
        self.records = []  # (tag, work, start_event, end_event)
        self.only = None if only is None else frozenset(only)   # bracket these operator tags only (None: every operator)
        self.agg = {}

    def fold(self):
        """Turn the recorded event pairs into per-operator totals and release the events.  Called whenever MAX_LIVE pairs are
        alive: with thousands of live timing events the HIP runtime stalled the host ONCE for 55-77 ms inside an event / launch
        call (tools/host_gap_probe.py: an eager Modified3DUNet run of 8 bracketed steps, ~1 250 events in), which an 8-step table
        then showed as a 7-8 ms-per-step bracket on whatever tiny operator happened to be inside."""
        if not self.records:
            return
        torch.cuda.synchronize()
        for tag, work, e0, e1 in self.records:
            a = self.agg.setdefault(tag, {"ms": 0.0, "calls": 0, "work": work})
            a["ms"] += e0.elapsed_time(e1)
            a["calls"] += 1
        self.records.clear()

    def summary(self):
        self.fold()
        return {k: dict(v) for k, v in self.agg.items()}


_timer = None


def set_timer(t):
    global _timer
    _timer = t


_roctx = None


def set_roctx(enabled=True):
    """roctx ranges around every C-ABI call: `rocprofv3 --marker-trace` then shows one range per operator, named
    like the bench's operator tags.  Off by default (a range costs two library calls per operator)."""
    global _roctx
    if not enabled:
        _roctx = None
        return
    h = ctypes.CDLL("libroctx64.so")
    h.roctxRangePushA.argtypes = [ctypes.c_char_p]
    h.roctxRangePushA.restype = ctypes.c_int
    h.roctxRangePop.restype = ctypes.c_int
    _roctx = h


class _timed:
    """with _timed(tag_fn, work_fn): <C-ABI call>  — tag_fn() names the operator, work_fn() = dict(flops=..., bytes=...)
    algorithmic figures per call; both are only evaluated when a timer or roctx is installed (no string formatting on the
    normal path)."""

    __slots__ = ("tag_fn", "work_fn", "e0", "tag")

    def __init__(self, tag_fn, work_fn=None):
        self.tag_fn, self.work_fn = tag_fn, work_fn

    def __enter__(self):
        if _timer is None and _roctx is None:
            self.e0 = None
            return
        self.tag = self.tag_fn()
        if _roctx is not None:
            _roctx.roctxRangePushA(self.tag.encode())
        self.e0 = None
        if _timer is not None and (_timer.only is None or self.tag in _timer.only):
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if _timer is not None and self.e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _timer.records.append((self.tag, self.work_fn() if self.work_fn is not None else None, self.e0, e1))
            if len(_timer.records) >= _timer.MAX_LIVE:
                _timer.fold()
        if _roctx is not None:
            _roctx.roctxRangePop()
        return False


def _conv_tag(kind, g):
    def axes(a, b, c):   # "2" for an isotropic stride / dilation, "2x1x1" otherwise
        return "%d" % a if a == b == c else "%dx%dx%d" % (a, b, c)
    return "conv3d_%s %dx%dx%d s%s d%s %d->%d @%dx%dx%d n%d%s" % (kind, g.kd, g.kh, g.kw, axes(g.sd, g.sh, g.sw),
                                                               axes(g.dd, g.dh, g.dw), g.ci, g.co, g.dout, g.ho, g.wo, g.n,
                                                               " bf16" if g.dtype == BF16 else "")


def _conv_work(g, kind):
    flops = 2.0 * g.n * g.co * g.ci * g.kd * g.kh * g.kw * g.dout * g.ho * g.wo
    esz = 2.0 if g.dtype == BF16 else 4.0
    xin = esz * g.n * g.di * g.hi * g.wi * g.ci
    yout = esz * g.n * g.dout * g.ho * g.wo * g.co
    wts = 4.0 * g.co * g.ci * g.kd * g.kh * g.kw
    return {"flops": flops, "bytes": xin + yout + wts}


def _triple(v):
    if isinstance(v, (tuple, list)):
        if len(v) == 1:
            return (int(v[0]),) * 3
        return tuple(int(a) for a in v)
    return (int(v),) * 3


# ----------------------------------------------------------------------------------------------- conv


def _conv_geom(xshape, wshape, stride, padding, dilation, x_ld=None, y_ld=None, dtype=F32):
    n, ci, di, hi, wi = xshape
    co, ci_w, kd, kh, kw = wshape
    if ci_w != ci:
        raise RuntimeError("conv3d: weight expects %d input channels, input has %d (groups are not supported)" % (ci_w, ci))
    sd, sh, sw = stride
    pd, ph, pw = padding
    dd, dh, dw = dilation
    do = (di + 2 * pd - dd * (kd - 1) - 1) // sd + 1
    ho = (hi + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    wo = (wi + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if do <= 0 or ho <= 0 or wo <= 0:
        raise RuntimeError("Kernel size can't be greater than actual input size")
    return ConvGeom(n, di, hi, wi, ci, do, ho, wo, co, kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw,
                    ci if x_ld is None else x_ld, co if y_ld is None else y_ld, dtype)


def _ptr_align(*ts):
    """Largest power of two <= 16 dividing the base address of every given tensor (None entries are skipped)."""
    bits = 16
    for t in ts:
        if t is not None:
            bits |= t.data_ptr()
    return bits & -bits


def conv_route(g, pass_, stats=False, bias=False, split=0, second_ld=0, align=16, x_align=None, y_align=None):
    """Name of the kernel the C ABI launches for geometry `g` (a ConvGeom from `_conv_geom`) in pass `pass_` (PASS_*): host only,
    nothing is launched and no device is needed.  split > 0: the *_cat entry points.  x_align / y_align: `_ptr_align` of the x-side
    tensor (x, or dx in the data gradient) and of the y-side tensor (y, or dy); `align` is the shorthand for both (16: what the
    allocator gives).  The vocabulary of names is documented at mri3d_conv3d_route in include/mri3d.h."""
    name = ctypes.create_string_buffer(64)
    xa, ya = align if x_align is None else x_align, align if y_align is None else y_align
    check(_lib.lib().mri3d_conv3d_route(ctypes.byref(g), pass_, int(bool(stats)), int(bool(bias)), split, second_ld, xa, ya, name, 64),
          "conv3d_route")
    return name.value.decode()


def pool_route(g, pass_, addend_ld=0, align=16, idx_align=16):
    """Name of the kernel max_pool3d launches for the PoolGeom `g` in pass `pass_` (PASS_FWD, PASS_DGRAD; addend_ld: the pitch of
    max_pool3d_skip's second gradient), host only, as `conv_route`.  align / idx_align: `_ptr_align` of the tensors / of the index
    bytes.  The vocabulary is documented at mri3d_maxpool3d_route in include/mri3d.h."""
    name = ctypes.create_string_buffer(64)
    check(_lib.lib().mri3d_maxpool3d_route(ctypes.byref(g), pass_, addend_ld, align, idx_align, name, 64), "maxpool3d_route")
    return name.value.decode()


def upsample_route(g, pass_, align=16):
    """Name of the kernel upsample3d launches for the UpGeom `g` in pass `pass_` (PASS_FWD, PASS_DGRAD), host only, as `conv_route`
    (vocabulary: mri3d_upsample3d_route in include/mri3d.h)."""
    name = ctypes.create_string_buffer(64)
    check(_lib.lib().mri3d_upsample3d_route(ctypes.byref(g), pass_, align, name, 64), "upsample3d_route")
    return name.value.decode()


RESAMPLE_PLAN_FIELDS = ("vec", "npv", "hch", "grid", "segs", "segl", "tiles_h", "tiles_w", "passes", "items", "tables", "lds_bytes")


def _resample_plan_dict(info):
    return {f: int(getattr(info, f)) for f in RESAMPLE_PLAN_FIELDS}


def pool_plan(g, pass_, addend_ld=0, align=16, idx_align=16):
    """Numbers of the launch plan whose kernel `pool_route` names (same arguments, host only): a dict of the fields of
    Mri3dResamplePlanInfo (include/mri3d.h)."""
    info = _lib.ResamplePlanInfo()
    check(_lib.lib().mri3d_maxpool3d_plan_query(ctypes.byref(g), pass_, addend_ld, align, idx_align, ctypes.byref(info)),
          "maxpool3d_plan_query")
    return _resample_plan_dict(info)


def upsample_plan(g, pass_, align=16):
    """Numbers of the launch plan whose kernel `upsample_route` names (same arguments, host only): a dict of the fields of
    Mri3dResamplePlanInfo (include/mri3d.h)."""
    info = _lib.ResamplePlanInfo()
    check(_lib.lib().mri3d_upsample3d_plan_query(ctypes.byref(g), pass_, align, ctypes.byref(info)), "upsample3d_plan_query")
    return _resample_plan_dict(info)


FUSEDCONV_PLAN_FIELDS = ("hch", "grid", "gtrips", "trips", "per", "passes", "chunks", "slabs", "rows")


def upconv_plan(g, scale, pass_):
    """Numbers of the launch plan of mri3d_upconv3d_fwd / _dgrad / _wgrad (PASS_FWD / PASS_DGRAD / PASS_WGRAD) for the ConvGeom `g`
    on the virtual fine input and the scale, host only: a dict of the fields of Mri3dFusedConvPlanInfo (include/mri3d.h)."""
    info = _lib.FusedConvPlanInfo()
    check(_lib.lib().mri3d_upconv3d_plan_query(ctypes.byref(g), scale, pass_, ctypes.byref(info)), "upconv3d_plan_query")
    return {f: int(getattr(info, f)) for f in FUSEDCONV_PLAN_FIELDS}


def conv_pair_plan(first, second):
    """Numbers of the launch plan of mri3d_convpair_wgrad_first for the two ConvGeoms, host only: a dict of the fields of
    Mri3dFusedConvPlanInfo (include/mri3d.h)."""
    info = _lib.FusedConvPlanInfo()
    check(_lib.lib().mri3d_convpair_plan_query(ctypes.byref(first), ctypes.byref(second), ctypes.byref(info)), "convpair_plan_query")
    return {f: int(getattr(info, f)) for f in FUSEDCONV_PLAN_FIELDS}


MARCH_PLAN_FIELDS = ("chunks", "blocks", "wgh", "wgw", "gch", "gcw", "nseg", "seglen", "nbuf", "grid", "whole_chunks", "dispatcher",
                     "smem_bytes", "wp_bytes")


def conv_march_plan(g, pass_, stats=False):
    """Numbers of the launch plan of mri3d_conv3d_fwd_march / _dgrad_march (PASS_FWD / PASS_DGRAD; stats: the forward with fused
    statistics) for the ConvGeom `g`, host only: a dict of the fields of Mri3dMarchPlanInfo (include/mri3d.h)."""
    info = _lib.MarchPlanInfo()
    check(_lib.lib().mri3d_conv3d_march_plan_query(ctypes.byref(g), pass_, 1 if stats else 0, ctypes.byref(info)),
          "conv3d_march_plan_query")
    return {f: int(getattr(info, f)) for f in MARCH_PLAN_FIELDS}


MFMA_PLAN_FIELDS = tuple(f for f, _ in _lib.ConvMfmaPlanInfo._fields_)
MFMA_KERNELS = {1: "tiled", 2: "tiled_n8", 3: "direct", 4: "cin1", 5: "wgrad3", 6: "wgrad4", 7: "bf16", 8: "bf16t", 9: "wgrad6"}


def conv_mfma_plan(g, pass_, stats=False, bias=False, split=0, second_ld=0, align=16, x_align=None, y_align=None):
    """Numbers of the launch plan whose kernel `conv_route` names (same arguments, host only) where the 3x3x3 MFMA kernels of
    csrc/conv_mfma.hip / conv_mfma_wgrad.hip serve the call: a dict of the fields of Mri3dConvMfmaPlanInfo (include/mri3d.h), `kernel`
    as the first word of the route name.  Raises Mri3dError (MRI3D_ENOTSUP) where `conv_route` names another file's kernel or "none"."""
    info = _lib.ConvMfmaPlanInfo()
    xa, ya = align if x_align is None else x_align, align if y_align is None else y_align
    check(_lib.lib().mri3d_conv3d_mfma_plan_query(ctypes.byref(g), pass_, int(bool(stats)), int(bool(bias)), split, second_ld, xa, ya,
                                                  ctypes.byref(info)), "conv3d_mfma_plan_query")
    out = {f: int(getattr(info, f)) for f in MFMA_PLAN_FIELDS}
    out["kernel"] = MFMA_KERNELS[out["kernel"]]
    return out


def norm_plan(g, pass_, align=16):
    """Launch plan of the norm-activation family for geometry `g` (a NormGeom) in pass `pass_` (NORM_PASS_STATS / _FWD / _BWD): the
    tuple (vec, CL, VT, cy, nblk, groups, gvox) documented at mri3d_norm_plan_query in include/mri3d.h.  Host only: nothing is
    launched and no device is needed.  align: `_ptr_align` of the tensors the pass touches (x; x and y; x, dy and dx)."""
    info = NormPlanInfo()
    check(_lib.lib().mri3d_norm_plan_query(ctypes.byref(g), pass_, align, ctypes.byref(info)), "norm_plan_query")
    return (info.vec, info.CL, info.VT, info.cy, info.nblk, info.groups, info.gvox)


def _stuffed_wgrad_ok(g):
    return ((g.kd, g.kh, g.kw) == (3, 3, 3) and (g.sd, g.sh, g.sw) == (2, 2, 2) and (g.pd, g.ph, g.pw) == (1, 1, 1)
            and (g.dd, g.dh, g.dw) == (1, 1, 1) and g.ci % 8 == 0 and g.co % 4 == 0 and g.x_ld % 4 == 0)


_ONE = (1, 1, 1)
_ConvPasses = collections.namedtuple("_ConvPasses", "fwd dgrad wgrad stuffed layer")


def _conv_passes(xshape, wshape, stride, padding, dilation, dtype=F32, x_ld=None, dy_ld=None, dx_ld=None):
    """The geometries of a convolution layer's three passes: the one place they are built, read by the operators and by the route
    queries alike.  The layer: x of logical shape xshape and voxel pitch x_ld, an incoming gradient of pitch dy_ld, a data gradient
    written with pitch dx_ld (None: dense, as y always is).  stuffed: where `_stuffed_wgrad_ok`, the stride-1 geometry the weight
    gradient runs on instead of wgrad (its gradient operand is then the dense tensor `_stuffed_wgrad` makes), else None."""
    fwd = _conv_geom(xshape, wshape, stride, padding, dilation, x_ld=x_ld, dtype=dtype)
    dgrad = _conv_geom(xshape, wshape, stride, padding, dilation, x_ld=dx_ld, y_ld=dy_ld, dtype=dtype)
    wgrad = _conv_geom(xshape, wshape, stride, padding, dilation, x_ld=fwd.x_ld, y_ld=dy_ld, dtype=dtype)
    stuffed = _conv_geom(xshape, wshape, _ONE, _ONE, _ONE, x_ld=fwd.x_ld, dtype=dtype) if _stuffed_wgrad_ok(fwd) else None
    return _ConvPasses(fwd, dgrad, wgrad, stuffed, (tuple(xshape), tuple(wshape), stride, padding, dilation, dtype, x_ld, dx_ld))


def _for_gradient_pitch(p, dy_ld):
    """p's layer for an incoming gradient of pitch dy_ld: p itself where built for it (forward builds for a dense one, the usual)."""
    return p if dy_ld == p.wgrad.y_ld else _conv_passes(*p.layer[:7], dy_ld=dy_ld, dx_ld=p.layer[7])


def _cat_passes(xa, xb, wshape, a_ld, dy_ld=None):
    """conv3d_cat's layer: 3x3x3 / stride 1 / pad 1 over the channels of xa (pitch a_ld) then xb's; two dense data gradients."""
    ca = xa.shape[1]
    return _conv_passes((xa.shape[0], ca + xb.shape[1]) + tuple(xa.shape[2:]), wshape, _ONE, _ONE, _ONE, _dt(xa), a_ld, dy_ld, dx_ld=ca)


def _upconv_passes(xshape, wshape, scale, padding, dtype, x_ld, dy_ld=None):
    """upsample_conv3d's layer: stride 1 over the nearest-upsampled grid, which x (pitch x_ld) is read through."""
    n, c, d, h, w = xshape
    return _conv_passes((n, c, d * scale, h * scale, w * scale), wshape, _ONE, padding, _ONE, dtype, x_ld, dy_ld)


def _pair_passes(xshape, x_ld, dtype, w1shape, conv1, w2shape, conv2):
    """conv3d_pair's layers: (the first, the second on the first's dense result); conv1 / conv2: modules like nn.Conv3d."""
    g1 = _conv_passes(xshape, w1shape, _triple(conv1.stride), _triple(conv1.padding), _ONE, dtype, x_ld).fwd
    return g1, _conv_passes((g1.n, g1.co, g1.dout, g1.ho, g1.wo), w2shape, _triple(conv2.stride), _triple(conv2.padding), _ONE, dtype)


def _transpose_geom(xshape, wshape, stride, padding, output_padding, dilation, dtype):
    """The mirrored convolution conv_transpose3d runs on: x is its output, the result (extents settled by output_padding) its input."""
    out = tuple((i - 1) * s - 2 * p + d * (k - 1) + op + 1 for i, s, p, d, k, op in zip(xshape[2:], stride, padding, dilation, wshape[2:], output_padding))
    g = _conv_geom((xshape[0], wshape[1]) + out, wshape, stride, padding, dilation, dtype=dtype)
    if (g.dout, g.ho, g.wo) != tuple(xshape[2:]):
        raise RuntimeError("conv_transpose3d: inconsistent output_padding")
    return g


def conv3d_routes(xshape, wshape, stride=1, padding=0, dilation=1, dtype=F32, x_ld=None, dy_ld=None, bias=True, bn_stats=False,
                  x_align=16, dy_align=16):
    """{"fwd": name, "dgrad": name, "wgrad": name} of the kernels `conv3d(x, w, b, ...)` and its backward launch, read from the
    `_conv_passes` that `_Conv3dFn` launches by: x a slice of pitch x_ld, the incoming gradient one of pitch dy_ld, y and dx fresh
    dense tensors (16-byte aligned), no bias in the data gradient, the stride-2 weight gradient on the stride-1 kernels where the
    passes say so (for tensors of one dtype, as `_stuffed_wgrad` asks).  *_align: `_ptr_align` of x / of the incoming gradient.  With
    bn_stats the forward name is that of the fused-statistics entry point where it serves the geometry (as `conv3d(bn_stats=True)`
    asks first)."""
    p = _conv_passes(xshape, wshape, _triple(stride), _triple(padding), _triple(dilation), dtype, x_ld, dy_ld)
    fwd = conv_route(p.fwd, PASS_FWD, bn_stats, bias, x_align=x_align, y_align=16) if bn_stats else "none"
    if fwd == "none":
        fwd = conv_route(p.fwd, PASS_FWD, False, bias, x_align=x_align, y_align=16)
    gw, wy_align = (p.wgrad, dy_align) if p.stuffed is None else (p.stuffed, 16)
    return {"fwd": fwd, "dgrad": conv_route(p.dgrad, PASS_DGRAD, x_align=16, y_align=dy_align),
            "wgrad": conv_route(gw, PASS_WGRAD, x_align=x_align, y_align=wy_align)}


def conv_transpose3d_routes(xshape, wshape, stride=1, padding=0, output_padding=0, dilation=1, dtype=F32, bias=True, x_align=16,
                            dy_align=16):
    """{"fwd": name, "dgrad": name, "wgrad": name} of the kernels `conv_transpose3d(x, w, b, ...)` and its backward launch, read
    from the `_transpose_geom` that `_ConvTranspose3dFn` launches by (dense tensors): the forward is the mirrored convolution's data
    gradient with the bias, dx its forward without one, dw its weight gradient with the operands swapped.  *_align: `_ptr_align` of
    x / of the incoming gradient."""
    g = _transpose_geom(xshape, wshape, _triple(stride), _triple(padding), _triple(output_padding), _triple(dilation), dtype)
    return {"fwd": conv_route(g, PASS_DGRAD, False, bias, x_align=16, y_align=x_align),
            "dgrad": conv_route(g, PASS_FWD, x_align=dy_align, y_align=16),
            "wgrad": conv_route(g, PASS_WGRAD, x_align=dy_align, y_align=x_align)}


def _carg(a):   # a tensor (or None) as its address, a geometry by reference, anything else as it is
    return _ptr(a) if a is None or torch.is_tensor(a) else ctypes.byref(a) if isinstance(a, ctypes.Structure) else a


def _launch(fn, tag, work, ws_bytes, device, *args):
    """The launch tail of the convolution, pool and upsample operators: the stream's workspace of ws_bytes (None: the entry point
    takes none), the `_timed(tag, work)` bracket and the checked call fn(*args, workspace, its size, stream), fn an entry point of
    the library."""
    tail = ()
    if ws_bytes is not None:
        ws = _workspace(ws_bytes, device)
        tail = (_ptr(ws), ws.numel())
    with _timed(tag, work):
        rc = fn(*map(_carg, args), *tail, _stream())
        if rc != 0:
            check(rc, fn.__name__[len("mri3d_"):])


def _conv_launch(fn, pass_, g, device, *args, suffix=""):
    """`_launch` of a convolution entry point fn(g, *args, ...) for pass `pass_`: the pass's workspace, tag (+ suffix) and work."""
    kind = ("fwd", "dgrad", "wgrad")[pass_]       # (PASS_FWD, PASS_DGRAD, PASS_WGRAD)
    _launch(fn, lambda: _conv_tag(kind, g) + suffix, lambda: _conv_work(g, kind),
            _lib.lib().mri3d_conv3d_workspace_bytes(ctypes.byref(g), pass_), device, g, *args)


def _conv_fwd(g, x, w, b, part=None):
    """y = conv(x, w) + b of geometry g.  part: the statistics partials of `_stats_partials`, for the epilogue to fill."""
    y = _new((g.n, g.co, g.dout, g.ho, g.wo), x)
    if part is None:
        _conv_launch(_lib.lib().mri3d_conv3d_fwd, PASS_FWD, g, x.device, x, w, b, y)
    else:
        _conv_launch(_lib.lib().mri3d_conv3d_fwd_stats, PASS_FWD, g, x.device, x, w, b, y, part, suffix=" +bn-stats")
    return y


def _conv_dgrad(g, dy, w, b, like):
    dx = _new((g.n, g.ci, g.di, g.hi, g.wi), like)
    _conv_launch(_lib.lib().mri3d_conv3d_dgrad, PASS_DGRAD, g, dy.device, dy, w, b, dx)
    return dx


class GradSink:
    """Where a parameter's gradient lives when `parallel.FlatParams` owns it: a view into the flat gradient buffer.  The
    backward of every op here writes a parameter gradient STRAIGHT into that view the first time the parameter is used after
    `FlatParams.zero_grad()` (later uses add to it) and hands autograd `None`, so there is no AccumulateGrad `add_` kernel per
    parameter per step (59 of them in the c0=8 U-Net).

    Contract (what a caller of an attached model can rely on):
      * `loss.backward()` behaves as usual: afterwards `p.grad` holds the accumulated gradient.
      * Zero gradients with `FlatParams.zero_grad()` (or the engine's step objects).  `flat.grad.zero_()` / `p.grad.zero_()` are
        also correct — the sink then ADDS into the zeroed view instead of overwriting it — just one `add_` slower.
      * The sink cannot tell `backward()` from `torch.autograd.grad(loss, params)` or `backward(inputs=[...])`: under those it
        would still write into `p.grad` and hand autograd None.  Code that wants gradient TENSORS of attached parameters
        (gradient penalties, inspection) wraps that call in `with ops.suspend_grad_sinks():` — the ops then return their
        parameter gradients to autograd like any other function."""

    __slots__ = ("view", "fresh")

    def __init__(self, view):
        self.view, self.fresh = view, True


_sinks_suspended = 0


class suspend_grad_sinks:
    """Context manager: inside it every op returns its parameter gradients to autograd (see GradSink's contract)."""

    def __enter__(self):
        global _sinks_suspended
        _sinks_suspended += 1
        return self

    def __exit__(self, *exc):
        global _sinks_suspended
        _sinks_suspended -= 1
        return False


def _live_sink(param):
    """param's sink if it is still what param.grad points at (a caller may have dropped or replaced .grad), else None."""
    if _sinks_suspended:
        return None
    sink = getattr(param, "_mri3d_grad_sink", None) if param is not None else None
    if sink is None or param.grad is None or param.grad.data_ptr() != sink.view.data_ptr() or sink.view.shape != param.shape:
        return None
    return sink


def _sink_take(param):
    """The sink view to write into if `param` has a fresh one (and mark it used), else None."""
    sink = _live_sink(param)
    if sink is None or not sink.fresh:
        return None
    sink.fresh = False
    return sink.view


def _sink_done(param, grad, out):
    """What backward returns for `param`: None when the gradient went (or now goes) into its sink, else the tensor."""
    if grad is None or out is not None:
        return None
    sink = _live_sink(param)
    if sink is None or sink.view.shape != grad.shape:
        return grad
    sink.view.add_(grad)      # second use of a shared parameter in this step, or a step without zero_grad()
    return None


def _grad_slots(ctx, saved, first=1, params=None, all_written=False):
    """(sinks, grads) for the parameter gradients a backward kernel writes.  saved: what forward kept of `params` (ctx.params
    unless given), inputs first.. of the function, None where a gradient cannot exist.  A wanted gradient goes to its fresh sink
    view, else to a new tensor.  all_written: the kernel writes every gradient that can exist, wanted or not, so each gets a
    tensor.  That is the rule of the convolutions' weight-gradient kernels: dw is computed even when only db is wanted, and db is
    written whenever the layer HAS a bias (a NULL db would select another kernel instantiation); `_grad_slots_done` hands
    autograd the wanted ones."""
    params = ctx.params if params is None else params
    want = [t is not None and ctx.needs_input_grad[first + i] for i, t in enumerate(saved)]
    sinks = [_sink_take(p) if wt else None for p, wt in zip(params, want)]
    grads = [(sk if sk is not None else torch.empty_like(t, memory_format=torch.contiguous_format))
             if wt or (all_written and t is not None) else None for sk, t, wt in zip(sinks, saved, want)]
    return sinks, grads


def _grad_slots_done(ctx, grads, sinks, first=1, params=None):
    """What backward returns for the parameters of `_grad_slots`."""
    params = ctx.params if params is None else params
    return tuple(_sink_done(p, gr, sk) if ctx.needs_input_grad[first + i] else None for i, (p, gr, sk) in enumerate(zip(params, grads, sinks)))


def _conv_param_grads(ctx, first, params, wgrad):
    """(dw, db) as backward returns them for the convolution whose (weight, bias) `params` are inputs first, first + 1 of the
    function: (None, None) unless one of them is wanted, else `wgrad(dw, db)` fills the tensors of `_grad_slots`."""
    if not any(p is not None and ctx.needs_input_grad[first + i] for i, p in enumerate(params)):
        return None, None
    sinks, grads = _grad_slots(ctx, params, first, params, all_written=True)
    wgrad(*grads)
    return _grad_slots_done(ctx, grads, sinks, first, params)


def _conv_wgrad(g, x, dy, w_like, want_bias, dw_out=None, db_out=None, split=None):
    """split: (xb, ca, b_ld) of conv3d_cat — x holds the first ca channels of the operand, xb (pitch b_ld) the others."""
    L = _lib.lib()
    dw = dw_out if dw_out is not None else torch.empty_like(w_like, memory_format=torch.contiguous_format)
    db = (db_out if db_out is not None else torch.empty(g.co, dtype=w_like.dtype, device=w_like.device)) if want_bias else None
    if split is None:
        _conv_launch(L.mri3d_conv3d_wgrad, PASS_WGRAD, g, x.device, x, dy, dw, db)
    else:
        _conv_launch(L.mri3d_conv3d_wgrad_cat, PASS_WGRAD, g, x.device, x, *split, dy, dw, db, suffix=" cat")
    return dw, db


def _stuffed_wgrad(p, x, dy):
    """(geometry, incoming gradient) the weight gradient of the passes `p` runs on: (p.wgrad, dy) as given, except where
    `_stuffed_wgrad_ok` and the two tensors share a dtype."""
    if p.stuffed is None or dy.dtype != x.dtype:
        return p.wgrad, dy
    # 3x3x3 / stride 2 / pad 1 (modified_3dunet.py:23-38): dW[tap] = sum_o X[2o - 1 + tap] dY[o] is the STRIDE-1 weight
    # gradient of X against dY spread onto the even voxels of a zero volume — 8x the arithmetic, but on the MFMA
    # weight-gradient kernel (~100 TFLOP/s) instead of the generic one (4.6 TFLOP/s on the 8 -> 16 layer at 80x96x80)
    g = p.fwd
    dyw = torch.empty((g.n, g.co, g.di, g.hi, g.wi), dtype=dy.dtype, device=dy.device, memory_format=CL3D).zero_()
    dyw[:, :, ::2, ::2, ::2].copy_(dy)
    return p.stuffed, dyw


def _autocast_in(x):
    """The activation input x in the storage dtype of the active `autocast` region (x itself outside one)."""
    return convert(x, _autocast_dtype) if _autocast_dtype is not None and x.dtype != _autocast_dtype else x


def _stats_partials(holder, blocks, g, x, bias):
    """BatchNorm follows in batch-statistics mode: the conv epilogue accumulates sum(a), sum(a^2) per output channel (float64
    partials, one per workgroup) instead of a statistics pass over y afterwards.  Returns the partials for the `blocks` workgroups
    the statistics query answered (None for 0: the kernel does not serve the geometry) and hands them to `holder`."""
    if blocks <= 0:
        return None
    part = torch.empty(blocks * g.co * 2, dtype=torch.float64, device=x.device)
    holder.append((part, blocks, bias.detach() if bias is not None else None))
    return part


def _apply_with_bn_stats(fn, bn_stats, *args):
    """fn.apply(*args, holder): with bn_stats the result carries the statistics its forward handed to holder (`_stats_partials`),
    where `norm_act` picks them up."""
    holder = [] if bn_stats else None
    y = fn.apply(*args, holder)
    if holder:
        y._mri3d_bn_stats = holder[0]
    return y


class _Conv3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, dilation, stats_holder=None):
        _require_device(x)
        _require_param(weight, bias)
        x, x_ld = _nd(x)
        w = weight.contiguous()
        p = _conv_passes(x.shape, w.shape, stride, padding, dilation, _dt(x), x_ld)
        g = p.fwd
        part = _stats_partials(stats_holder, _lib.lib().mri3d_conv3d_fwd_stats_blocks(ctypes.byref(g)), g, x, bias) if stats_holder is not None else None
        y = _conv_fwd(g, x, w, bias, part)
        ctx.save_for_backward(x, w)
        ctx.passes, ctx.params = p, (weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy, y_ld = _nd(dy)
        p = _for_gradient_pitch(ctx.passes, y_ld)
        dx = _conv_dgrad(p.dgrad, dy, w, None, x) if ctx.needs_input_grad[0] else None      # a fresh dense tensor (pitch = Cin)

        def wgrad(dw, db):
            gw, dyw = _stuffed_wgrad(p, x, dy)
            _conv_wgrad(gw, x, dyw, w, db is not None, dw, db)
        return (dx, *_conv_param_grads(ctx, 1, ctx.params, wgrad), None, None, None, None)


class _Conv3dCatFn(torch.autograd.Function):
    """conv3d(torch.cat((xa, xb), dim=1), w, b, padding=1) for a 3x3x3 kernel WITHOUT the concatenation: the MFMA kernels read the
    two tensors chunk by chunk (mri3d_conv3d_fwd_cat / _wgrad_cat) and the data gradient comes out as two dense tensors
    (mri3d_conv3d_dgrad_cat).  unet.UNet decoder: cat((skip, upsampled)) -> ConvolutionalBlock (segmentation/routine.py:346-356).
    Writing a 16-channel slice of a 48-channel NDHWC buffer costs 1.5x (fp32) to 3.6x (bf16) of a dense write
    (tools/slice_write_probe.py), which is what the copy-free concat buffer of round 1 made its producers do."""

    @staticmethod
    def forward(ctx, xa, xb, weight, bias, stats_holder=None):
        _require_device(xa, xb)
        _require_param(weight, bias)
        L = _lib.lib()
        xa, a_ld = _nd(xa)
        xb, b_ld = _nd(xb)
        w = weight.contiguous()
        p = _cat_passes(xa, xb, w.shape, a_ld)
        g, ca = p.fwd, xa.shape[1]
        y = _new((g.n, g.co, g.dout, g.ho, g.wo), xa)
        ws_bytes = L.mri3d_conv3d_workspace_bytes(ctypes.byref(g), PASS_FWD)
        part = None
        if stats_holder is not None:
            # the partials are sized by the query about exactly what is launched: geometry, split and second-tensor pitch (the
            # pitch takes part in the choice between the marching and the tiled kernel, whose grids differ)
            part = _stats_partials(stats_holder, L.mri3d_conv3d_fwd_cat_stats_blocks(ctypes.byref(g), ca, b_ld), g, xa, bias)
        _launch(L.mri3d_conv3d_fwd_cat, lambda: _conv_tag("fwd", g) + " cat" + (" +bn-stats" if part is not None else ""),
                lambda: _conv_work(g, "fwd"), ws_bytes, xa.device, g, xa, xb, ca, b_ld, w, bias, y, part)
        ctx.save_for_backward(xa, xb, w)
        ctx.passes, ctx.b_ld, ctx.params = p, b_ld, (weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        xa, xb, w = ctx.saved_tensors
        dy, y_ld = _nd(dy)
        p = _for_gradient_pitch(ctx.passes, y_ld)
        ca, cb = xa.shape[1], xb.shape[1]
        dxa = dxb = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dxa, dxb = _new(xa.shape, xa), _new(xb.shape, xb)      # two dense tensors
            _conv_launch(_lib.lib().mri3d_conv3d_dgrad_cat, PASS_DGRAD, p.dgrad, dy.device, dy, w, dxa, dxb, ca, cb, suffix=" cat")
        dw, db = _conv_param_grads(ctx, 2, ctx.params, lambda dw, db: _conv_wgrad(p.wgrad, xa, dy, w, db is not None, dw, db,
                                                                                 split=(xb, ca, ctx.b_ld)))
        return dxa, dxb, dw, db, None


def conv3d_cat(xa, xb, weight, bias=None, padding=1, bn_stats=False):
    """conv3d(torch.cat((xa, xb), dim=1), weight, bias, padding=padding) — without the concatenation where the MFMA kernels serve all
    three passes of the geometry (3x3x3 / stride 1 / pad 1, channel counts in multiples of 16), with an explicit one otherwise."""
    xa, xb = _autocast_in(xa), _autocast_in(xb)
    ok = (xa.is_cuda and xa.dim() == 5 and xb.shape[0] == xa.shape[0] and xb.shape[2:] == xa.shape[2:] and xa.dtype == xb.dtype
          and tuple(weight.shape[2:]) == (3, 3, 3) and _triple(padding) == (1, 1, 1) and weight.shape[1] == xa.shape[1] + xb.shape[1])
    if ok:
        L = _lib.lib()
        a_nd, a_ld = _nd(xa)
        b_nd, b_ld = _nd(xb)
        ca, cb = xa.shape[1], xb.shape[1]
        p = _cat_passes(a_nd, b_nd, weight.shape, a_ld)
        ok = (a_nd.data_ptr() % 16 == 0 and b_nd.data_ptr() % 16 == 0
              and L.mri3d_conv3d_cat_supported(ctypes.byref(p.fwd), ca, b_ld, PASS_FWD)
              and L.mri3d_conv3d_cat_supported(ctypes.byref(p.fwd), ca, b_ld, PASS_WGRAD)
              and L.mri3d_conv3d_cat_supported(ctypes.byref(p.dgrad), ca, cb, PASS_DGRAD))
    if not ok:
        return conv3d(cat_channels([xa, xb]), weight, bias, 1, padding, 1, bn_stats=bn_stats)
    return _apply_with_bn_stats(_Conv3dCatFn, bn_stats, xa, xb, weight, bias)


def conv3d(x, weight, bias=None, stride=1, padding=0, dilation=1, bn_stats=False):
    """bn_stats=True: the caller applies a batch-statistics BatchNorm to the result next (nn.conv_norm_act); where the MFMA
    forward kernel serves the geometry its epilogue accumulates the statistics, and `norm_act` picks them up from the result."""
    return _apply_with_bn_stats(_Conv3dFn, bn_stats, _autocast_in(x), weight, bias, _triple(stride), _triple(padding), _triple(dilation))


# ----------------------------------------------------------------------------------------------- first layer + activation
# unet.UNet's first ConvolutionalBlock: Conv3d(1, 8, 3, padding=1) + PReLU, nothing in between.  One autograd node on two kernels
# (mri3d_conv_cin1_act_fwd / _bwd) instead of conv, activation, activation backward and weight gradient: the pre-activation z is
# stored once and its gradient never.


def conv_cin1_act_route(g, a_ld, act_code, alpha_n, pass_, align=16):
    """Name of the kernel mri3d_conv_cin1_act_fwd (PASS_FWD) / _bwd (PASS_WGRAD) launches for the convolution g, "none" where the
    native predicate declines: host only, nothing is launched and no device is needed."""
    name = ctypes.create_string_buffer(64)
    check(_lib.lib().mri3d_conv_cin1_act_route(ctypes.byref(g), a_ld, act_code, alpha_n, pass_, align, name, 64), "conv_cin1_act_route")
    return name.value.decode()


def _cin1_act_alpha_n(act_code, alpha):
    return 1 if act_code != ACT_PRELU else (alpha.numel() if alpha is not None else 0)


def conv3d_act_supported(x, weight, act, alpha=None, out=None):
    """True when `conv3d_act` serves act(conv3d(x, weight, bias, padding=1)) as one operator: what only the caller can see (an fp32
    tensor outside an autocast region whose own gradient nobody wants, an NDHWC layout, an activation with a slope), then the
    native predicate on the geometry.  Host only: it answers for host tensors too."""
    if not (torch.is_tensor(x) and x.dim() == 5 and x.dtype == torch.float32 and not x.requires_grad):
        return False
    if _autocast_dtype is not None or act not in ("relu", "leaky_relu", "prelu"):
        return False
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or weight.shape[1] != x.shape[1] or weight.dtype != torch.float32:
        return False
    if act == "prelu" and (alpha is None or alpha.dtype != torch.float32):
        return False
    x_ld = _pitch_of(x)
    g = _conv_geom(x.shape, weight.shape, _ONE, _ONE, _ONE, x_ld=x.shape[1] if x_ld is None else x_ld)
    act_code = _ACT_CODES[act]
    z_ld = a_ld = g.co
    if out is not None:
        z_ld, a_ld = _pitch_of(out[0]), _pitch_of(out[1])
        if z_ld is None or a_ld is None:
            return False
        g.y_ld = z_ld
    align = 16 if out is None else _ptr_align(*out)
    return bool(_lib.lib().mri3d_conv_cin1_act_supported(ctypes.byref(g), a_ld, act_code, _cin1_act_alpha_n(act_code, alpha), PASS_FWD, align))


def _cin1_act_tag(kind, g):
    return "conv3d_act_%s 1->%d @%dx%dx%d n%d" % (kind, g.co, g.dout, g.ho, g.wo, g.n)


class _Conv3dActFn(torch.autograd.Function):
    """a = act(z), z = conv3d(x, weight, bias, padding=1), for one input channel.  Saves x and z; the backward forms the gradient of
    z in registers.  out: None, or (z, a) to write into (logical (N, Co, D, H, W) tensors of NDHWC memory, any pitch)."""

    @staticmethod
    def forward(ctx, x, weight, bias, alpha, act, slope, out):
        _require_device(x)
        _require_param(weight, bias, alpha)
        L = _lib.lib()
        x, x_ld = _nd(x)
        w = weight.contiguous()
        g = _conv_geom(x.shape, w.shape, _ONE, _ONE, _ONE, x_ld=x_ld)
        shape = (g.n, g.co, g.dout, g.ho, g.wo)
        z, a = (_new(shape, x), _new(shape, x)) if out is None else out
        if tuple(z.shape) != shape or tuple(a.shape) != shape or z.dtype != x.dtype or a.dtype != x.dtype:
            raise RuntimeError("conv3d_act(out=): two float32 tensors of shape %s expected" % (shape,))
        g.y_ld, a_ld = _pitch_of(z), _pitch_of(a)
        if g.y_ld is None or a_ld is None:
            raise RuntimeError("conv3d_act(out=): the output tensors must be NDHWC in memory")
        act_code = _ACT_CODES[act]
        prelu = act_code == ACT_PRELU
        alpha_n = _cin1_act_alpha_n(act_code, alpha)
        _launch(L.mri3d_conv_cin1_act_fwd, lambda: _cin1_act_tag("fwd", g),
                lambda: {"flops": _conv_work(g, "fwd")["flops"], "bytes": 4.0 * (x.numel() + 2 * z.numel())},
                L.mri3d_conv_cin1_act_workspace_bytes(ctypes.byref(g), PASS_FWD), x.device,
                g, a_ld, act_code, alpha_n, float(slope), x, w, bias, alpha if prelu else None, z, a)
        ctx.save_for_backward(x, w, z, alpha if prelu else None)
        ctx.geom, ctx.act, ctx.slope = g, (act_code, alpha_n), float(slope)
        ctx.params, ctx.has_bias = (weight, bias, alpha if prelu else None), bias is not None
        return a

    @staticmethod
    def backward(ctx, da):
        L = _lib.lib()
        x, w, z, alpha = ctx.saved_tensors
        g0 = ctx.geom
        act_code, alpha_n = ctx.act
        if da.dtype != z.dtype:
            raise RuntimeError("conv3d_act backward: gradient dtype %s does not match activation dtype %s" % (da.dtype, z.dtype))
        if ctx.needs_input_grad[0]:
            raise RuntimeError("conv3d_act: no data gradient (ops.conv3d_act_supported declines an input that requires one)")
        weight, bias, alpha_p = ctx.params
        if not any(p is not None and ctx.needs_input_grad[1 + i] for i, p in enumerate(ctx.params)):
            return None, None, None, None, None, None, None
        da, da_ld = _nd(da)
        csinks, cgrads = _grad_slots(ctx, (w, bias), 1, (weight, bias), all_written=True)
        asinks, agrads = _grad_slots(ctx, (alpha,), 3, (alpha_p,))
        dw, db = cgrads
        dalpha = agrads[0]
        g = _repitched(g0, g0.x_ld, g0.y_ld)
        if L.mri3d_conv_cin1_act_supported(ctypes.byref(g), da_ld, act_code, alpha_n, PASS_WGRAD, _ptr_align(z, da)):
            _launch(L.mri3d_conv_cin1_act_bwd, lambda: _cin1_act_tag("bwd", g),
                    lambda: {"flops": _conv_work(g, "wgrad")["flops"], "bytes": 4.0 * (x.numel() + 2 * z.numel())},
                    L.mri3d_conv_cin1_act_workspace_bytes(ctypes.byref(g), PASS_WGRAD), x.device,
                    g, da_ld, act_code, alpha_n, ctx.slope, x, z, da, alpha, dw, db, dalpha)
        else:
            # where the backward kernel is not offered (sixteen output channels: the layer's weight gradient is an MFMA kernel
            # with its own summation order): the activation's backward and the plain weight gradient, as without the fold
            zd = z if g0.y_ld == g0.co else z.contiguous(memory_format=CL3D)
            dz = _new(zd.shape, zd)
            ng = NormGeom(g0.n, g0.dout * g0.ho * g0.wo, g0.co, g0.co, da_ld, 0, act_code, alpha_n, ctx.slope, 0.0, 0, F32)
            ws = _workspace(L.mri3d_norm_workspace_bytes(ctypes.byref(ng)), x.device)
            with _timed(lambda: "norm_act_bwd c%d vox%d n%d" % (ng.c, ng.vox, ng.n), lambda: {"flops": 0.0, "bytes": 20.0 * zd.numel()}):
                check(L.mri3d_norm_act_bwd(ctypes.byref(ng), 0, _ptr(zd), _ptr(da), None, None, None, None, _ptr(alpha), _ptr(dz), None,
                                           None, _ptr(dalpha), _ptr(ws), ws.numel(), _stream()), "norm_act_bwd")
            _conv_wgrad(_repitched(g0, g0.x_ld, g0.co), x, dz, w, db is not None, dw, db)
        return (None, *_grad_slots_done(ctx, cgrads, csinks, 1, (weight, bias)), *_grad_slots_done(ctx, agrads, asinks, 3, (alpha_p,)),
                None, None, None)


def conv3d_act(x, weight, bias=None, alpha=None, act="prelu", slope=0.01, out=None):
    """act(conv3d(x, weight, bias, padding=1)) for a 3x3x3 kernel over ONE input channel and act = "prelu" (alpha: one slope or one
    per channel), "leaky_relu" (slope) or "relu", as one operator — where `conv3d_act_supported`; a RuntimeError elsewhere (the
    caller keeps ops.conv3d + ops.norm_act).  out = (z, a): tensors to write the pre-activation and the result into."""
    if not conv3d_act_supported(x, weight, act, alpha, out):
        raise RuntimeError("conv3d_act: not served for this input, kernel or activation (ask conv3d_act_supported)")
    return _Conv3dActFn.apply(x, weight, bias, alpha, act, slope, out)


# ----------------------------------------------------------------------------------------------- BayesConv3d
# 3d_bayes_layers.py:195-232.  Two autograd nodes: the weight transform (parameters only, one small kernel each way) and the layer
# itself — two convolutions on the convolution kernels plus the streaming passes of csrc/bayes.hip.


class _BayesWeightsFn(torch.autograd.Function):
    """(mu, logsigma) -> (w_var, log_alpha) in train mode, (w_mean, w_var, log_alpha) in eval mode (mri3d_bayes_weights_*)."""

    @staticmethod
    def forward(ctx, mu, logsigma, evaluate, threshold):
        _require_param(mu, logsigma)
        if mu.shape != logsigma.shape:
            raise RuntimeError("bayes_conv3d: mu_weight %s and logsigma_weight %s differ in shape" % (tuple(mu.shape), tuple(logsigma.shape)))
        mu, logsigma = mu.contiguous(), logsigma.contiguous()
        w_var, log_alpha = torch.empty_like(mu), torch.empty_like(mu)
        w_mean = torch.empty_like(mu) if evaluate else None
        check(_lib.lib().mri3d_bayes_weights_fwd(_ptr(mu), _ptr(logsigma), mu.numel(), int(evaluate), float(threshold), _ptr(w_mean),
                                                 _ptr(w_var), _ptr(log_alpha), _stream()), "bayes_weights_fwd")
        ctx.save_for_backward(mu, logsigma)
        ctx.evaluate, ctx.threshold = bool(evaluate), float(threshold)
        ctx.set_materialize_grads(False)      # an unused output (log_alpha without a regulariser) arrives as None -> NULL
        return (w_mean, w_var, log_alpha) if evaluate else (w_var, log_alpha)

    @staticmethod
    def backward(ctx, *grads):
        mu, logsigma = ctx.saved_tensors
        d_w_mean, d_w_var, d_log_alpha = grads if ctx.evaluate else (None,) + grads
        d_w_mean, d_w_var, d_log_alpha = (None if g is None else g.contiguous() for g in (d_w_mean, d_w_var, d_log_alpha))
        dmu, dls = torch.empty_like(mu), torch.empty_like(mu)
        check(_lib.lib().mri3d_bayes_weights_bwd(_ptr(mu), _ptr(logsigma), mu.numel(), int(ctx.evaluate), ctx.threshold, _ptr(d_w_mean),
                                                 _ptr(d_w_var), _ptr(d_log_alpha), _ptr(dmu), _ptr(dls), _stream()),
              "bayes_weights_bwd")
        return dmu, dls, None, None


def _stream_work(n_tensors, like, eps_numel=0):
    return {"flops": 0.0, "bytes": _esz(like) * n_tensors * like.numel() + 4.0 * eps_numel}


def _bayes_square(x, x_ld):
    n, c, d, h, w = x.shape
    x2 = _new(x.shape, x)
    _launch(_lib.lib().mri3d_bayes_square, lambda: "bayes_square %d @%dx%dx%d n%d" % (c, d, h, w, n), lambda: _stream_work(2, x), None, None,
            x, x2, n * d * h * w, c, x_ld, c, _dt(x))
    return x2


class _BayesConv3dFn(torch.autograd.Function):
    """y = conv3d(x, w_mean, mu_bias) + eps * sqrt(1e-4 + conv3d(x^2, w_var, logsigma_bias^2)).  eps: float32, logical
    (N, Co, D, H, W), no gradient.  Backward (dvar = dy eps / (2 sqrt(1e-4 + var_out))):
        dx = dgrad(dy, w_mean) + 2 x dgrad(dvar, w_var)      dw_mean = wgrad(x, dy)      dw_var = wgrad(x^2, dvar)
        dmu_bias = sum dy      dlogsigma_bias = 2 logsigma_bias sum dvar
    x^2 is recomputed in the backward (one streaming pass) rather than kept alive between the passes."""

    @staticmethod
    def forward(ctx, x, w_mean, w_var, mu_bias, logsigma_bias, eps, stride, padding, dilation):
        _require_device(x)
        _require_param(w_mean, w_var, mu_bias, logsigma_bias, eps)
        L = _lib.lib()
        x, x_ld = _nd(x)
        w_mean, w_var = w_mean.contiguous(), w_var.contiguous()
        pm = _conv_passes(x.shape, w_mean.shape, stride, padding, dilation, _dt(x), x_ld)     # the mean reads x where it lies,
        pv = _conv_passes(x.shape, w_var.shape, stride, padding, dilation, _dt(x))            # the variance a dense x^2 (and dvar)
        g = pm.fwd
        y = _conv_fwd(g, x, w_mean, mu_bias)
        var_bias = logsigma_bias * logsigma_bias if logsigma_bias is not None else None
        var_out = _conv_fwd(pv.fwd, _bayes_square(x, x_ld), w_var, var_bias)
        if tuple(eps.shape) != tuple(y.shape):
            raise RuntimeError("bayes_conv3d: eps has shape %s, the output %s" % (tuple(eps.shape), tuple(y.shape)))
        eps, eps_ld = _nd(eps)
        nvox = g.n * g.dout * g.ho * g.wo
        _launch(L.mri3d_bayes_sample_fwd, lambda: "bayes_sample_fwd %d @%dx%dx%d n%d" % (g.co, g.dout, g.ho, g.wo, g.n),
                lambda: _stream_work(3, y, eps.numel()), None, None, y, var_out, eps, y, nvox, g.co, g.co, g.co, eps_ld, g.co, g.dtype)
        ctx.save_for_backward(x, w_mean, w_var, var_out, eps, logsigma_bias)
        ctx.passes, ctx.eps_ld, ctx.has_bias = (pm, pv), eps_ld, mu_bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, w_mean, w_var, var_out, eps, logsigma_bias = ctx.saved_tensors
        dy, y_ld = _nd(dy)
        pm, pv = _for_gradient_pitch(ctx.passes[0], y_ld), ctx.passes[1]
        g = pm.fwd
        nvox = g.n * g.dout * g.ho * g.wo
        dvar = _new(dy.shape, dy)
        _launch(L.mri3d_bayes_sample_bwd, lambda: "bayes_sample_bwd %d @%dx%dx%d n%d" % (g.co, g.dout, g.ho, g.wo, g.n),
                lambda: _stream_work(3, dy, eps.numel()), None, None, dy, var_out, eps, dvar, nvox, g.co, y_ld, g.co, ctx.eps_ld, g.co, g.dtype)
        dx = dw_mean = dw_var = dmb = dlb = None
        if ctx.needs_input_grad[0]:
            dx = _conv_dgrad(pm.dgrad, dy, w_mean, None, x)
            dx_var = _conv_dgrad(pv.dgrad, dvar, w_var, None, x)
            _launch(L.mri3d_bayes_dx, lambda: "bayes_dx %d @%dx%dx%d n%d" % (g.ci, g.di, g.hi, g.wi, g.n), lambda: _stream_work(4, x), None, None,
                    dx, dx_var, x, dx, g.n * g.di * g.hi * g.wi, g.ci, g.ci, g.ci, g.x_ld, g.ci, g.dtype)
        want_b = ctx.has_bias and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2] or want_b:
            gw, dyw = _stuffed_wgrad(pm, x, dy)
            dw_mean, dmb = _conv_wgrad(gw, x, dyw, w_mean, ctx.has_bias)
            gw2, dvw = _stuffed_wgrad(pv, x, dvar)
            dw_var, dvb = _conv_wgrad(gw2, _bayes_square(x, g.x_ld), dvw, w_var, ctx.has_bias)
            if ctx.has_bias:
                dlb = 2.0 * logsigma_bias * dvb
        return dx, dw_mean, dw_var, dmb, dlb, None, None, None, None


def bayes_conv3d(x, mu_weight, logsigma_weight, mu_bias=None, logsigma_bias=None, stride=1, padding=0, dilation=1, training=True,
                 threshold=3, eps=None, groups=1):
    """BayesConv3d.forward (3d_bayes_layers.py:210-232) -> (y, log_alpha).  `eps`: the standard-normal noise as a float32 device tensor
    of y's logical shape (N, Co, D, H, W); None draws it from torch's default device generator in y's NDHWC memory order, as
    `dropout3d` draws its mask.  The noise is sampled in train AND eval mode; eval mode masks the weights with
    log_alpha < threshold.  Under `autocast` x is converted like `conv3d` converts it, eps stays float32."""
    if groups != 1:
        raise NotImplementedError("bayes_conv3d: groups != 1 is not supported")
    if isinstance(padding, str):
        raise NotImplementedError("bayes_conv3d: string padding is not supported")
    if (mu_bias is None) != (logsigma_bias is None):
        raise RuntimeError("bayes_conv3d: mu_bias and logsigma_bias come together")
    _require_device(x)
    x = _autocast_in(x)
    stride, padding, dilation = _triple(stride), _triple(padding), _triple(dilation)
    g = _conv_geom(x.shape, mu_weight.shape, stride, padding, dilation)
    if training:
        w_mean = mu_weight
        w_var, log_alpha = _BayesWeightsFn.apply(mu_weight, logsigma_weight, False, threshold)
    else:
        w_mean, w_var, log_alpha = _BayesWeightsFn.apply(mu_weight, logsigma_weight, True, threshold)
    if eps is None:
        eps = torch.empty((g.n, g.dout, g.ho, g.wo, g.co), dtype=torch.float32, device=x.device).normal_().permute(0, 4, 1, 2, 3)
    y = _BayesConv3dFn.apply(x, w_mean, w_var, mu_bias, logsigma_bias, eps.detach(), stride, padding, dilation)
    return y, log_alpha


class _ConvPairFn(torch.autograd.Function):
    """y = conv3d(conv3d(x, w1, b1, stride s1, padding p1), w2, b2, stride s2, padding p2) for the head of the autoencoder's first
    DownBlock (AE_model.py:45-53: (6,1,1) on the one-channel input, then (1,k,1)), x a network input (no gradient).  Forward = the two
    convolutions; backward never forms the gradient of the intermediate tensor: w1's gradient comes from dy, w2 and x
    (mri3d_convpair_wgrad_first, csrc/sepconv.hip)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, conv1, conv2):
        _require_device(x)
        _require_param(w1, b1)
        _require_param(w2, b2)
        x, x_ld = _nd(x)
        w1c, w2c = w1.contiguous(), w2.contiguous()
        g1, p2 = _pair_passes(x.shape, x_ld, _dt(x), w1c.shape, conv1, w2c.shape, conv2)
        a1 = _conv_fwd(g1, x, w1c, b1)
        y = _conv_fwd(p2.fwd, a1, w2c, b2)
        ctx.save_for_backward(x, a1, w2c)
        ctx.passes, ctx.params = (g1, p2), (w1, b1, w2, b2)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, a1, w2c = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        dy, y_ld = _nd(dy)
        g1, gw2 = ctx.passes[0], _for_gradient_pitch(ctx.passes[1], y_ld).wgrad
        # second convolution: the ordinary weight gradient
        dw2, db2 = _conv_param_grads(ctx, 3, (w2, b2), lambda dw, db: _conv_wgrad(gw2, a1, dy, w2c, db is not None, dw, db))

        # first convolution: from dy, w2 and x, without the gradient of a1
        def wgrad_first(dw, db):
            _launch(L.mri3d_convpair_wgrad_first, lambda: _conv_tag("wgrad", g1) + " through " + _conv_tag("dgrad", gw2),
                    lambda: {"flops": _conv_work(g1, "wgrad")["flops"] + _conv_work(gw2, "dgrad")["flops"],
                             "bytes": _esz(dy) * (x.numel() + dy.numel())},
                    L.mri3d_convpair_workspace_bytes(ctypes.byref(g1), ctypes.byref(gw2)), x.device, g1, gw2, x, dy, w2c, dw, db)
        dw1, db1 = _conv_param_grads(ctx, 1, (w1, b1), wgrad_first)
        return None, dw1, db1, dw2, db2, None, None


def conv3d_pair_supported(x, conv1, conv2):
    """True when conv2(conv1(x)) is served by _ConvPairFn: x needs no gradient and mri3d_convpair_supported takes the pair.
    conv1 / conv2: modules with weight, bias, stride, padding, dilation (nn.Conv3d)."""
    if not (torch.is_tensor(x) and x.dim() == 5 and x.is_cuda) or x.requires_grad or _autocast_dtype is not None:
        return False
    if _triple(conv1.dilation) != (1, 1, 1) or _triple(conv2.dilation) != (1, 1, 1) or conv1.weight.shape[1] != x.shape[1]:
        return False
    try:
        g1, p2 = _pair_passes(x.shape, _pitch_of(x) or x.shape[1], _dt(x), conv1.weight.shape, conv1, conv2.weight.shape, conv2)
    except RuntimeError:
        return False
    return bool(_lib.lib().mri3d_convpair_supported(ctypes.byref(g1), ctypes.byref(p2.fwd)))


def conv3d_pair(x, conv1, conv2):
    """conv2(conv1(x)) for two nn.Conv3d modules; the fused backward where conv3d_pair_supported, else the two operators."""
    if conv3d_pair_supported(x, conv1, conv2):
        return _ConvPairFn.apply(x, conv1.weight, conv1.bias, conv2.weight, conv2.bias, conv1, conv2)
    y = conv3d(x, conv1.weight, conv1.bias, conv1.stride, conv1.padding, conv1.dilation)
    return conv3d(y, conv2.weight, conv2.bias, conv2.stride, conv2.padding, conv2.dilation)


def _channel_sum(t):
    """sum over (N,D,H,W) per channel with the norm-statistics kernel (mean * count)."""
    L = _lib.lib()
    n, c, d, h, w = t.shape
    g = NormGeom(n, d * h * w, c, c, c, 0, ACT_NONE, 1, 0.0, 0.0, 0, _dt(t))
    mean = torch.empty(c, dtype=torch.float32, device=t.device)
    invstd = torch.empty(c, dtype=torch.float32, device=t.device)
    ws = _workspace(L.mri3d_norm_workspace_bytes(ctypes.byref(g)), t.device)
    check(L.mri3d_norm_stats(ctypes.byref(g), _ptr(t), _ptr(mean), _ptr(invstd), None, None, 0.0, _ptr(ws), ws.numel(),
                             _stream()), "norm_stats")
    return mean * float(n * d * h * w)


class _ConvTranspose3dFn(torch.autograd.Function):
    """y = conv_transpose3d(x, w, b): forward is the data-gradient kernel of the mirrored Conv3d."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, output_padding, dilation):
        _require_device(x)
        _require_param(weight, bias)
        x = _cl(x)
        w = weight.contiguous()  # (Cin_t, Cout_t, kd, kh, kw) == conv weight (Co=Cin_t, Ci=Cout_t)
        if w.shape[0] != x.shape[1]:
            raise RuntimeError("conv_transpose3d: weight expects %d input channels, got %d" % (w.shape[0], x.shape[1]))
        g = _transpose_geom(x.shape, w.shape, stride, padding, output_padding, dilation, _dt(x))
        y = _conv_dgrad(g, x, w, bias, x)
        ctx.save_for_backward(x, w)
        ctx.geom, ctx.has_bias = g, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        g = ctx.geom
        dy = _cl(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _conv_fwd(g, dy, w, None)
        if ctx.needs_input_grad[1]:
            dw, _ = _conv_wgrad(g, dy, x, w, False)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _channel_sum(dy)
        return dx, dw, db, None, None, None, None


def conv_transpose3d(x, weight, bias=None, stride=1, padding=0, output_padding=0, dilation=1):
    return _ConvTranspose3dFn.apply(_autocast_in(x), weight, bias, _triple(stride), _triple(padding), _triple(output_padding),
                                    _triple(dilation))


# ----------------------------------------------------------------------------------------------- norm + activation

_ACT_CODES = {None: ACT_NONE, "none": ACT_NONE, "relu": ACT_RELU, "leaky_relu": ACT_LEAKY, "prelu": ACT_PRELU}

# Synchronised BatchNorm (SURVEY §8e "parity mode"): when a reducer is installed, training-mode BatchNorm layers take their
# statistics over the GLOBAL batch of all data-parallel ranks, so that N ranks x 2 volumes reproduce the statistics of one
# device with 2N volumes.  A reducer is any object with `all_reduce(t)` returning the element-wise sum of the float64 tensor
# `t` over all ranks (parallel.SyncBatchNorm wraps torch.distributed; tests inject a fake).  Two tiny collectives per layer
# per step (2C+1 doubles forward, 2C doubles backward); the default stays local statistics.
_sync_bn_reducer = None


def set_sync_batchnorm(reducer):
    """Install (or, with None, remove) the reducer of synchronised BatchNorm; returns the previous one."""
    global _sync_bn_reducer
    prev, _sync_bn_reducer = _sync_bn_reducer, reducer
    return prev


def sync_batchnorm_reducer():
    return _sync_bn_reducer


def _sync_statistics(reducer, g, x, running_mean, running_var, momentum, eps):
    """(mean, invstd, count) over the global batch: local moments with the statistics kernel, summed over the ranks as
    (count, sum x, sum x^2) in float64; updates the running buffers with the reduced statistics."""
    c = g.c
    mean_l, invstd_l = _norm_statistics("norm_act", g, x, 1, "batch", None, None, momentum, eps, None)
    # Wire format: (count, sum(x - s), sum((x - s)^2)) per channel in float64, with the shift s = running_mean (the same on
    # every rank: the buffers start equal and are only ever updated by this code with the reduced statistics) or 0
    # without running statistics.  The local variance comes from the statistics kernel's own shifted float64 sums, so
    # nothing here subtracts two large numbers once s has followed the mean (|mean| >> std: a raw E[x^2] - mean^2
    # across ranks would lose mean^2/var digits).
    cnt_l = float(g.n * g.vox)
    shift = running_mean.detach().double() if running_mean is not None else torch.zeros(c, dtype=torch.float64, device=x.device)
    m64 = mean_l.double() - shift
    var_l = (1.0 / invstd_l.double() ** 2 - float(eps)).clamp_(min=0.0)
    pack = torch.cat([torch.full((1,), cnt_l, dtype=torch.float64, device=x.device), cnt_l * m64,
                      cnt_l * (var_l + m64 * m64)])
    pack = reducer.all_reduce(pack)
    cnt = pack[0]
    gm_s = pack[1:1 + c] / cnt
    gmean = gm_s + shift
    gvar = (pack[1 + c:] / cnt - gm_s * gm_s).clamp_(min=0.0)
    mean = gmean.to(torch.float32).contiguous()
    invstd = torch.rsqrt(gvar + float(eps)).to(torch.float32).contiguous()
    if running_mean is not None:
        with torch.no_grad():
            unb = gvar * (cnt / torch.clamp(cnt - 1.0, min=1.0))
            running_mean.mul_(1.0 - momentum).add_(momentum * gmean.to(running_mean.dtype))
            running_var.mul_(1.0 - momentum).add_(momentum * unb.to(running_var.dtype))
    return mean, invstd, cnt


def _sync_correct_dx(reducer, g, x, mean, invstd, gamma, dbeta, dgamma, cnt, dx):
    """dx += the two mean-subtraction terms of the BatchNorm gradient over the global batch.  The two batch sums (sum dy',
    sum dy' * xhat) are exactly what the kernel reported as d(beta), d(gamma) of the frozen-statistics formula: sum them over
    the ranks, then apply the terms as one more per-channel affine pass over x."""
    L = _lib.lib()
    tot = reducer.all_reduce(torch.cat([dbeta.double(), dgamma.double()]))
    gam = gamma.double() if gamma is not None else torch.ones(g.c, dtype=torch.float64, device=x.device)
    a0 = (-gam * invstd.double() * tot[:g.c] / cnt).to(torch.float32).contiguous()
    b1 = (-gam * invstd.double() ** 2 * tot[g.c:] / cnt).to(torch.float32).contiguous()
    ones = torch.ones(g.c, dtype=torch.float32, device=x.device)
    corr = _new(x.shape, x)
    ga = NormGeom(g.n, g.vox, g.c, g.c, g.c, 0, ACT_NONE, 1, 0.0, 0.0, 0, g.dtype)
    # corr = b1 * (x - mean) + a0, then dx += corr
    check(L.mri3d_norm_act_fwd(ctypes.byref(ga), _ptr(x), _ptr(mean), _ptr(ones), _ptr(b1), _ptr(a0), None, _ptr(corr),
                               _stream()), "norm_act_fwd")
    check(L.mri3d_add_channels(_ptr(dx), _ptr(corr), _ptr(dx), g.n * g.vox, g.c, g.c, g.c, g.c, g.dtype, _stream()),
          "add_channels")


def _norm_geom(x, x_ld, y_ld, act_code, alpha, slope, eps, instance=0, group_c=0):
    """NormGeom of act(norm(x)): voxel pitches x_ld (x / dx) and y_ld (the output / its gradient).  alpha_n counts PReLU's
    slopes; 0, which nothing serves, when PReLU comes without them."""
    n, c, d, h, w = x.shape
    alpha_n = 1 if act_code != ACT_PRELU else (alpha.numel() if alpha is not None else 0)
    return NormGeom(n, d * h * w, c, x_ld, y_ld, instance, act_code, alpha_n, float(slope), float(eps), group_c, _dt(x))


def _repitched(g, x_ld, y_ld, dtype=None):
    """A copy of the geometry g (NormGeom, PoolGeom or UpGeom) with other voxel pitches — what a backward pass makes of its
    forward's geometry — and, where given, the storage type of the gradient it reads."""
    g = type(g).from_buffer_copy(g)
    g.x_ld, g.y_ld = x_ld, y_ld
    if dtype is not None:
        g.dtype = dtype
    return g


def _norm_statistics(who, g, x, groups, mode, running_mean, running_var, momentum, eps, fused_stats):
    """(mean, invstd) per (group, channel) for mode "batch" (computed here; running buffers, where given, are updated), "running"
    (from the buffers) or "none" (None, None).  groups: 1, or the batch size for instance / group statistics; fused_stats: None,
    or the partials of the producing conv's epilogue."""
    if mode == "none":
        return None, None
    if mode == "running":
        return (running_mean.detach().to(torch.float32).contiguous(),
                torch.rsqrt(running_var.detach().to(torch.float32) + eps).contiguous())
    if mode != "batch":
        raise RuntimeError("%s: statistics mode %r is not served" % (who, mode))
    L = _lib.lib()
    c = g.c
    g = _repitched(g, g.x_ld, g.x_ld)   # the statistics entry points: y_ld is a pitch of c channels
    mean = torch.empty(groups * c, dtype=torch.float32, device=x.device)
    invstd = torch.empty(groups * c, dtype=torch.float32, device=x.device)
    if fused_stats is not None and fused_stats[0].numel() == fused_stats[1] * c * 2:
        # the producing conv's epilogue already summed (y - bias), (y - bias)^2 per channel: only the finalize kernel runs
        part, blocks, shift = fused_stats
        with _timed(lambda: "norm_stats(from conv partials) c%d" % c, lambda: {"flops": 0.0, "bytes": 8.0 * part.numel()}):
            check(L.mri3d_norm_stats_from_partials(ctypes.byref(g), _ptr(part), blocks, _ptr(shift), _ptr(mean), _ptr(invstd),
                                                   _ptr(running_mean), _ptr(running_var), float(momentum), _stream()),
                  "norm_stats_from_partials")
    else:
        ws = _workspace(L.mri3d_norm_workspace_bytes(ctypes.byref(g)), x.device)
        with _timed(lambda: "norm_stats c%d vox%d n%d" % (c, g.vox, g.n), lambda: {"flops": 0.0, "bytes": _esz(x) * x.numel()}):
            check(L.mri3d_norm_stats(ctypes.byref(g), _ptr(x), _ptr(mean), _ptr(invstd), _ptr(running_mean), _ptr(running_var),
                                     float(momentum), _ptr(ws), ws.numel(), _stream()), "norm_stats")
    return mean, invstd


def _fused_stats_of(x, stats_mode, momentum):
    """Prologue of the public wrappers: the fused BatchNorm statistics of x's producing conv, where x carries them."""
    if momentum is None:
        raise RuntimeError("cumulative moving average (momentum=None) is not supported")
    return getattr(x, "_mri3d_bn_stats", None) if stats_mode == "batch" else None


def _backward_x(who, x, g0, *grads):
    """x as the backward kernels read it, after checking the incoming gradients' dtype."""
    for t in grads:
        if t is not None and t.dtype != x.dtype:
            raise RuntimeError("%s backward: gradient dtype %s does not match activation dtype %s" % (who, t.dtype, x.dtype))
    if g0.x_ld != g0.c:  # dx shares x's pitch in the kernel: give it a dense x instead
        x = x.contiguous(memory_format=CL3D)
    return x


class _NormActFn(torch.autograd.Function):
    """y = act(gamma * (x - mean) / sqrt(var + eps) + beta) with batch, instance, running or no statistics."""

    @staticmethod
    def forward(ctx, x, gamma, beta, alpha, running_mean, running_var, stats_mode, momentum, eps, act, slope, out, group_c=0,
                fused_stats=None):
        # stats_mode: "batch" (compute + update running), "instance", "running" (eval BN), "none" (activation only)
        # out: None, or (buffer, channel_offset): write y into that channel slice of a wider NDHWC buffer
        _require_device(x)
        _require_param(gamma, beta, alpha)
        ctx.params = (gamma, beta, alpha)
        L = _lib.lib()
        x, x_ld = _nd(x)
        n, c, d, h, w = x.shape
        act_code = _ACT_CODES[act]
        instance = 1 if stats_mode in ("instance", "group") else 0
        if stats_mode == "group" and (group_c <= 0 or c % group_c):
            raise RuntimeError("group norm: channels per group %d must divide C=%d" % (group_c, c))
        group_c = group_c if stats_mode == "group" else 0
        if out is None:
            y, y_ld, y_off = _new(x.shape, x), c, 0
        else:
            buf, y_off = out
            y_ld = _pitch_of(buf)
            if (y_ld != buf.shape[1] or tuple(buf.shape[2:]) != (d, h, w) or buf.shape[0] != n or y_off + c > buf.shape[1]
                    or buf.dtype != x.dtype):
                raise RuntimeError("norm_act(out=): buffer %s cannot hold a %s slice at channel %d"
                                   % (tuple(buf.shape), tuple(x.shape), y_off))
            y = _slice_view(buf, y_off, c)
        g = _norm_geom(x, x_ld, y_ld, act_code, alpha, slope, eps, instance, group_c)
        ctx.training_stats = stats_mode in ("batch", "instance", "group")
        ctx.sync = _sync_bn_reducer if stats_mode == "sync" else None
        if stats_mode == "sync":
            if ctx.sync is None:
                raise RuntimeError("norm_act(stats_mode='sync') needs ops.set_sync_batchnorm(reducer)")
            mean, invstd, ctx.sync_count = _sync_statistics(ctx.sync, g, x, running_mean, running_var, momentum, eps)
        else:   # instance and group: batch statistics of n groups, without running buffers
            mode = "batch" if ctx.training_stats else (stats_mode if stats_mode == "running" else "none")
            mean, invstd = _norm_statistics("norm_act", g, x, n if instance else 1, mode, None if instance else running_mean,
                                            None if instance else running_var, momentum, eps, fused_stats)
        with _timed(lambda: "norm_act_fwd c%d vox%d n%d" % (c, g.vox, n), lambda: {"flops": 0.0, "bytes": 2 * _esz(x) * x.numel()}):
            check(L.mri3d_norm_act_fwd(ctypes.byref(g), _ptr(x), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta),
                                       _ptr(alpha) if act_code == ACT_PRELU else None, _ptr(y), _stream()),
                  "norm_act_fwd")
        ctx.save_for_backward(x, mean, invstd, gamma, beta, alpha)
        ctx.geom = g
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, mean, invstd, gamma, beta, alpha = ctx.saved_tensors
        g0 = ctx.geom
        dy, dy_ld = _nd(dy)
        x = _backward_x("norm_act", x, g0, dy)
        dx = _new(x.shape, x)
        g = _repitched(g0, g0.c, dy_ld)
        prelu = g.act == ACT_PRELU
        sinks, grads = _grad_slots(ctx, (gamma, beta, alpha if prelu else None))
        dgamma_k, dbeta_k, dalpha = grads
        sync = ctx.sync
        if sync is not None:
            # the kernel's d(gamma), d(beta) double as the batch sums of _sync_correct_dx: it writes them even where unwanted
            dbeta_k = dbeta_k if dbeta_k is not None else torch.empty(g.c, dtype=torch.float32, device=x.device)
            dgamma_k = dgamma_k if dgamma_k is not None else torch.empty(g.c, dtype=torch.float32, device=x.device)
        ws = _workspace(L.mri3d_norm_workspace_bytes(ctypes.byref(g)), x.device)
        with _timed(lambda: "norm_act_bwd c%d vox%d n%d" % (g.c, g.vox, g.n), lambda: {"flops": 0.0, "bytes": 5 * _esz(x) * x.numel()}):
            check(L.mri3d_norm_act_bwd(ctypes.byref(g), 1 if ctx.training_stats else 0, _ptr(x), _ptr(dy), _ptr(mean),
                                       _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(alpha) if prelu else None, _ptr(dx),
                                       _ptr(dgamma_k), _ptr(dbeta_k), _ptr(dalpha), _ptr(ws), ws.numel(), _stream()),
                  "norm_act_bwd")
        if sync is not None:
            _sync_correct_dx(sync, g, x, mean, invstd, gamma, dbeta_k, dgamma_k, ctx.sync_count, dx)
        return (dx, *_grad_slots_done(ctx, grads, sinks), None, None, None, None, None, None, None, None, None, None)


def norm_act(x, gamma=None, beta=None, alpha=None, running_mean=None, running_var=None, stats_mode="batch",
             momentum=0.1, eps=1e-5, act=None, slope=0.01, out=None, group_c=0):
    fused = _fused_stats_of(x, stats_mode, momentum)
    return _NormActFn.apply(x, gamma, beta, alpha, running_mean, running_var, stats_mode, momentum, eps, act, slope, out,
                            group_c, fused)


def _fusable_x_ld(x, stats_mode, act):
    """What the two `*_supported` predicates ask of x, the statistics and the activation before their native predicate: the
    pitch x will be read with, or None where the fused operators do not serve the call."""
    if stats_mode not in ("batch", "running", "none") or act not in _ACT_CODES:
        return None
    if not (x.dim() == 5 and x.dtype in (torch.float32, torch.bfloat16)):
        return None
    x_ld = _pitch_of(x)
    if x_ld is None:
        return x.shape[1]          # _nd makes a dense copy
    return None if x.data_ptr() % (4 * x.element_size()) else x_ld


def norm_act_pointwise_supported(x, weight, stats_mode="batch", act=None, alpha=None):
    """True when `norm_act_pointwise` serves act(norm(x)) followed by the 1x1x1 convolution `weight` (co, c, 1, 1, 1) as one
    operator: the native predicate on the geometry, plus what only the caller can see (statistics mode, memory layout)."""
    x_ld = _fusable_x_ld(x, stats_mode, act) if x.is_cuda else None
    if x_ld is None:
        return False
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (1, 1, 1) or weight.shape[1] != x.shape[1] or weight.dtype != torch.float32:
        return False
    g = _norm_geom(x, x_ld, weight.shape[0], _ACT_CODES[act], alpha, 0.0, 0.0)
    return bool(_lib.lib().mri3d_norm_act_pw_supported(ctypes.byref(g), weight.shape[0]))


class _NormActPointwiseFn(torch.autograd.Function):
    """logits = conv1x1x1(act(gamma * (x - mean) / sqrt(var + eps) + beta), weight, bias) with batch, running or no statistics:
    the activation between the two operators and its gradient are never stored (mri3d_norm_act_pw_*)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, alpha, weight, bias, running_mean, running_var, stats_mode, momentum, eps, act, slope,
                fused_stats=None):
        _require_device(x)
        _require_param(gamma, beta, alpha, weight, bias)
        ctx.params = (gamma, beta, alpha, weight, bias)
        L = _lib.lib()
        x, x_ld = _nd(x)
        n, c, d, h, w = x.shape
        co = weight.shape[0]
        act_code = _ACT_CODES[act]
        wm = weight.contiguous()
        g = _norm_geom(x, x_ld, co, act_code, alpha, slope, eps)
        if not L.mri3d_norm_act_pw_supported(ctypes.byref(g), co):
            raise RuntimeError("norm_act_pointwise: c=%d co=%d pitch %d is not served (ask norm_act_pointwise_supported first)"
                               % (c, co, x_ld))
        mean, invstd = _norm_statistics("norm_act_pointwise", g, x, 1, stats_mode, running_mean, running_var, momentum, eps,
                                        fused_stats)
        out = _new((n, co, d, h, w), x)
        with _timed(lambda: "norm_act_pw_fwd c%d->%d vox%d n%d" % (c, co, g.vox, n),
                    lambda: {"flops": 2.0 * co * c * n * g.vox, "bytes": _esz(x) * (x.numel() + out.numel())}):
            check(L.mri3d_norm_act_pw_fwd(ctypes.byref(g), co, _ptr(x), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta),
                                          _ptr(alpha) if act_code == ACT_PRELU else None, _ptr(wm), _ptr(bias), _ptr(out),
                                          _stream()), "norm_act_pw_fwd")
        ctx.save_for_backward(x, mean, invstd, gamma, beta, alpha, wm)
        ctx.geom = g
        ctx.training_stats = stats_mode == "batch"
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.lib()
        x, mean, invstd, gamma, beta, alpha, wm = ctx.saved_tensors
        g0 = ctx.geom
        co = wm.shape[0]
        dout, o_ld = _nd(dout)
        x = _backward_x("norm_act_pointwise", x, g0, dout)
        g = _repitched(g0, g0.c, o_ld)
        prelu = g.act == ACT_PRELU
        sinks, grads = _grad_slots(ctx, (gamma, beta, alpha if prelu else None, wm, ctx.params[4]))
        dx = _new(x.shape, x) if ctx.needs_input_grad[0] else None
        ws = _workspace(L.mri3d_norm_act_pw_workspace_bytes(ctypes.byref(g), co), x.device)
        # training statistics: x and dout are read twice and dx written once; frozen statistics: one read
        reads = 2 if ctx.training_stats else 1
        with _timed(lambda: "norm_act_pw_bwd c%d->%d vox%d n%d" % (g.c, co, g.vox, g.n),
                    lambda: {"flops": 4.0 * co * g.c * g.n * g.vox,
                             "bytes": _esz(x) * (reads * (x.numel() + dout.numel()) + (x.numel() if dx is not None else 0))}):
            check(L.mri3d_norm_act_pw_bwd(ctypes.byref(g), co, 1 if ctx.training_stats else 0, _ptr(x), _ptr(dout), _ptr(mean),
                                          _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(alpha) if prelu else None, _ptr(wm),
                                          _ptr(dx), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(grads[3]),
                                          _ptr(grads[4]), _ptr(ws), ws.numel(), _stream()), "norm_act_pw_bwd")
        return (dx, *_grad_slots_done(ctx, grads, sinks), None, None, None, None, None, None, None, None)


def norm_act_pointwise(x, weight, bias=None, gamma=None, beta=None, alpha=None, running_mean=None, running_var=None,
                       stats_mode="batch", momentum=0.1, eps=1e-5, act=None, slope=0.01):
    """conv3d(norm_act(x, ...), weight, bias) for a 1x1x1 `weight` with at most four output channels, as one operator (see
    `norm_act_pointwise_supported`); the producer's fused BatchNorm statistics are picked up from x as `norm_act` does."""
    fused = _fused_stats_of(x, stats_mode, momentum)
    return _NormActPointwiseFn.apply(x, gamma, beta, alpha, weight, bias, running_mean, running_var, stats_mode, momentum, eps,
                                     act, slope, fused)


def _pool_geom(x, s_ld, p_ld, kernel, stride, padding):
    """(PoolGeom, pooled extents) of a max pool over a tensor of x's shape — x itself, or the act(norm(x)) of `norm_act_pool`:
    voxel pitches s_ld (its input / that one's gradient) and p_ld (pooled / dpool)."""
    n, c, d, h, w = x.shape
    do, ho, wo = (_pool_out(i, k, s, p, False) for i, k, s, p in zip((d, h, w), kernel, stride, padding))
    return PoolGeom(n, d, h, w, do, ho, wo, c, *kernel, *stride, *padding, s_ld, p_ld, _dt(x)), (do, ho, wo)


def norm_act_pool_supported(x, kernel_size=2, stride=None, padding=0, stats_mode="batch", act=None, alpha=None):
    """True when `norm_act_pool` serves act(norm(x)) followed by max_pool3d_skip as one operator: the native predicate on the two
    geometries (a host-only decision: x may live anywhere), plus what only the caller can see (statistics mode, memory layout)."""
    x_ld = _fusable_x_ld(x, stats_mode, act)
    if x_ld is None:
        return False
    k = _triple(kernel_size)
    s = _triple(stride) if stride is not None else k
    c = x.shape[1]
    g = _norm_geom(x, x_ld, c, _ACT_CODES[act], alpha, 0.0, 0.0)
    pg, out = _pool_geom(x, c, c, k, s, _triple(padding))
    if min(out) <= 0:
        return False
    return bool(_lib.lib().mri3d_norm_act_pool_supported(ctypes.byref(g), ctypes.byref(pg)))


class _NormActPoolFn(torch.autograd.Function):
    """(pooled, skip) = (max_pool3d(a, 2), a) with a = act(gamma * (x - mean) / sqrt(var + eps) + beta), batch, running or no
    statistics: one forward pass writes a, the pooled tensor and the index bytes; the backward takes dskip + scatter(dpool) inside
    the norm_act backward passes and never stores it (mri3d_norm_act_pool_*)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, alpha, running_mean, running_var, stats_mode, momentum, eps, act, slope, fused_stats=None):
        _require_device(x)
        _require_param(gamma, beta, alpha)
        ctx.params = (gamma, beta, alpha)
        L = _lib.lib()
        x, x_ld = _nd(x)
        n, c, d, h, w = x.shape
        act_code = _ACT_CODES[act]
        two = (2, 2, 2)
        g = _norm_geom(x, x_ld, c, act_code, alpha, slope, eps)
        pg, (do, ho, wo) = _pool_geom(x, c, c, two, two, (0, 0, 0))
        if not L.mri3d_norm_act_pool_supported(ctypes.byref(g), ctypes.byref(pg)):
            raise RuntimeError("norm_act_pool: c=%d pitch %d extents %s is not served (ask norm_act_pool_supported first)"
                               % (c, x_ld, (d, h, w)))
        mean, invstd = _norm_statistics("norm_act_pool", g, x, 1, stats_mode, running_mean, running_var, momentum, eps,
                                        fused_stats)
        skip = _new(x.shape, x)
        pooled = _new((n, c, do, ho, wo), x)
        idx = torch.empty(pooled.numel(), dtype=torch.uint8, device=x.device)
        # read x; write skip, pooled and one index byte per pooled element
        with _timed(lambda: "norm_act_pool_fwd c%d" % c,
                    lambda: {"flops": 0.0, "bytes": _esz(x) * 2 * x.numel() + (_esz(x) + 1) * pooled.numel()}):
            check(L.mri3d_norm_act_pool_fwd(ctypes.byref(g), ctypes.byref(pg), _ptr(x), _ptr(mean), _ptr(invstd), _ptr(gamma),
                                            _ptr(beta), _ptr(alpha) if act_code == ACT_PRELU else None, _ptr(skip), _ptr(pooled),
                                            _ptr(idx), _stream()), "norm_act_pool_fwd")
        ctx.save_for_backward(x, idx, mean, invstd, gamma, beta, alpha)
        ctx.geom = g
        ctx.pooled_shape = tuple(pooled.shape)
        ctx.training_stats = stats_mode == "batch"
        ctx.set_materialize_grads(False)   # an unused output arrives as None and is not read as zeros
        return pooled, skip

    @staticmethod
    def backward(ctx, dpool, dskip):
        L = _lib.lib()
        if dpool is None and dskip is None:
            return (None,) * 12
        x, idx, mean, invstd, gamma, beta, alpha = ctx.saved_tensors
        g0 = ctx.geom
        n, c, d, h, w = x.shape
        s_ld = p_ld = c
        for name, t, shape in (("pooled", dpool, ctx.pooled_shape), ("skip", dskip, tuple(x.shape))):
            if t is not None and tuple(t.shape) != shape:
                raise RuntimeError("norm_act_pool backward: %s gradient %s does not match %s" % (name, tuple(t.shape), shape))
        if dskip is not None:
            dskip, s_ld = _nd(dskip)
            if s_ld % 4 or dskip.data_ptr() % (4 * dskip.element_size()):
                dskip, s_ld = dskip.contiguous(memory_format=CL3D), c
        if dpool is not None:
            dpool, p_ld = _nd(dpool)
            if p_ld % 4 or dpool.data_ptr() % (4 * dpool.element_size()):
                dpool, p_ld = dpool.contiguous(memory_format=CL3D), c
        x = _backward_x("norm_act_pool", x, g0, dpool, dskip)
        two = (2, 2, 2)
        g = _repitched(g0, c, s_ld)
        pg, _ = _pool_geom(x, s_ld, p_ld, two, two, (0, 0, 0))
        prelu = g.act == ACT_PRELU
        sinks, grads = _grad_slots(ctx, (gamma, beta, alpha if prelu else None))
        dx = _new(x.shape, x) if ctx.needs_input_grad[0] else None
        ws = _workspace(L.mri3d_norm_act_pool_workspace_bytes(ctypes.byref(g), ctypes.byref(pg)), x.device)
        # per pass: x and dskip read, dpool and the index bytes read once (each is shared by a window's eight voxels); training
        # statistics take the sums pass and the dx pass, frozen statistics one pass; dx written once
        passes = 2 if ctx.training_stats else 1
        npool = idx.numel()
        with _timed(lambda: "norm_act_pool_bwd c%d" % c,
                    lambda: {"flops": 0.0,
                             "bytes": passes * (_esz(x) * (x.numel() + (x.numel() if dskip is not None else 0))
                                                + ((_esz(x) + 1) * npool if dpool is not None else 0))
                                      + (_esz(x) * x.numel() if dx is not None else 0)}):
            check(L.mri3d_norm_act_pool_bwd(ctypes.byref(g), ctypes.byref(pg), 1 if ctx.training_stats else 0, _ptr(x),
                                            _ptr(dskip), _ptr(dpool), _ptr(idx), _ptr(mean), _ptr(invstd), _ptr(gamma),
                                            _ptr(beta), _ptr(alpha) if prelu else None, _ptr(dx), _ptr(grads[0]), _ptr(grads[1]),
                                            _ptr(grads[2]), _ptr(ws), ws.numel(), _stream()), "norm_act_pool_bwd")
        return (dx, *_grad_slots_done(ctx, grads, sinks), None, None, None, None, None, None, None, None)


def norm_act_pool(x, gamma=None, beta=None, alpha=None, running_mean=None, running_var=None, stats_mode="batch",
                  momentum=0.1, eps=1e-5, act=None, slope=0.01):
    """(max_pool3d(a, 2), a) for a = norm_act(x, ...) as one operator (see `norm_act_pool_supported`): the second output is the
    skip connection's tensor.  The producer's fused BatchNorm statistics are picked up from x as `norm_act` does."""
    fused = _fused_stats_of(x, stats_mode, momentum)
    return _NormActPoolFn.apply(x, gamma, beta, alpha, running_mean, running_var, stats_mode, momentum, eps, act, slope, fused)


def activation(x, act, alpha=None, slope=0.01):
    return norm_act(x, None, None, alpha, None, None, "none", 0.1, 0.0, act, slope)


class _ScaleInstanceFn(torch.autograd.Function):
    """y[n,c,...] = x[n,c,...] * scale[n,c]  (Dropout3d mask application, modified_3dunet.py:12)."""

    @staticmethod
    def forward(ctx, x, scale):
        _require_device(x)
        _require_param(scale)
        L = _lib.lib()
        x = _cl(x)
        n, c, d, h, w = x.shape
        g = NormGeom(n, d * h * w, c, c, c, 1, ACT_NONE, 1, 0.0, 0.0, 0, _dt(x))
        scale = scale.reshape(n * c).contiguous()
        zeros = torch.zeros_like(scale)
        y = _new(x.shape, x)
        check(L.mri3d_norm_act_fwd(ctypes.byref(g), _ptr(x), _ptr(zeros), _ptr(scale), None, None, None, _ptr(y),
                                   _stream()), "norm_act_fwd")
        ctx.save_for_backward(scale, zeros)
        ctx.geom = g
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        scale, zeros = ctx.saved_tensors
        g = ctx.geom
        dy = _cl(dy)
        dx = _new(dy.shape, dy)
        check(L.mri3d_norm_act_fwd(ctypes.byref(g), _ptr(dy), _ptr(zeros), _ptr(scale), None, None, None, _ptr(dx),
                                   _stream()), "norm_act_fwd")
        return dx, None


def dropout3d(x, p, training):
    """Channel dropout: the Bernoulli mask is N*C numbers drawn by torch's generator; the volume pass is HIP."""
    if not training or p == 0.0:
        return x
    n, c = x.shape[0], x.shape[1]
    keep = torch.empty(n, c, device=x.device, dtype=torch.float32).bernoulli_(1.0 - p)
    return _ScaleInstanceFn.apply(x, keep / (1.0 - p))


# ----------------------------------------------------------------------------------------------- pooling


def _pool_out(i, k, s, p, ceil_mode):
    if ceil_mode:
        o = -(-(i + 2 * p - k) // s) + 1
        if (o - 1) * s >= i + p:
            o -= 1
        return o
    return (i + 2 * p - k) // s + 1


class _MaxPool3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        _require_device(x)
        x, x_ld = _nd(x)
        n, c, d, h, w = x.shape
        g, (do, ho, wo) = _pool_geom(x, x_ld, c, kernel, stride, padding)
        if do <= 0 or ho <= 0 or wo <= 0:
            raise RuntimeError("max_pool3d: output size is too small (input %s, kernel %s)" % ((d, h, w), kernel))
        y = _new((n, c, do, ho, wo), x)
        idx = torch.empty(n * do * ho * wo * c, dtype=torch.uint8, device=x.device)
        _launch(_lib.lib().mri3d_maxpool3d_fwd, lambda: "maxpool_fwd c%d" % c,
                lambda: {"flops": 0.0, "bytes": _esz(x) * x.numel() + (_esz(x) + 1) * y.numel()}, None, x.device, g, x, y, idx)
        ctx.save_for_backward(idx)
        ctx.geom = g
        ctx.xshape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        return _pool_backward(ctx, dy)


def _pool_backward(ctx, dy, dskip=None, ds_ld=0):
    """dx = maxpool_bwd(dy), plus dskip (the other gradient of x, NDHWC with voxel pitch ds_ld) where `_MaxPoolSkipFn` has one."""
    (idx,) = ctx.saved_tensors
    dy, dy_ld = _nd(dy)
    dx = _new(ctx.xshape, dy)
    g = _repitched(ctx.geom, ctx.geom.c, dy_ld, _dt(dy))
    if dskip is None:
        _launch(_lib.lib().mri3d_maxpool3d_bwd, lambda: "maxpool_bwd c%d" % g.c,
                lambda: {"flops": 0.0, "bytes": _esz(dy) * dx.numel() + (_esz(dy) + 1) * dy.numel()}, None, dy.device, g, dy, idx, dx)
    else:
        _launch(_lib.lib().mri3d_maxpool3d_bwd_add, lambda: "maxpool_bwd+skip c%d" % g.c,
                lambda: {"flops": 0.0, "bytes": _esz(dy) * 2 * dx.numel() + (_esz(dy) + 1) * dy.numel()}, None, dy.device,
                g, dy, idx, dskip, ds_ld, dx)
    return dx, None, None, None


class _MaxPoolSkipFn(torch.autograd.Function):
    """`skip = x; y = max_pool3d(x)` as ONE autograd node returning (y, skip): the encoder output feeds both the pool and
    the decoder's skip connection (unet.UNet encoder blocks), so its gradient is maxpool_bwd(dy) + dskip — summed inside the
    pool-backward kernel instead of by a separate full-resolution autograd add (0.48 ms per step on the 16-channel level)."""

    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        y = _MaxPool3dFn.forward(ctx, x, kernel, stride, padding)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dskip):
        if dskip is None:
            return _MaxPool3dFn.backward(ctx, dy)
        if dy is None:
            return dskip, None, None, None
        dskip, ds_ld = _nd(dskip)
        if tuple(dskip.shape) != ctx.xshape or dskip.dtype != dy.dtype:
            raise RuntimeError("max_pool3d_skip backward: skip gradient %s %s does not match the input %s %s"
                               % (tuple(dskip.shape), dskip.dtype, ctx.xshape, dy.dtype))
        return _pool_backward(ctx, dy, dskip, ds_ld)


def max_pool3d_skip(x, kernel_size, stride=None, padding=0):
    """(max_pool3d(x), x): use the second output for the skip connection so that both gradients meet in one kernel."""
    k = _triple(kernel_size)
    s = _triple(stride) if stride is not None else k
    return _MaxPoolSkipFn.apply(x, k, s, _triple(padding))


def max_pool3d(x, kernel_size, stride=None, padding=0):
    k = _triple(kernel_size)
    s = _triple(stride) if stride is not None else k
    return _MaxPool3dFn.apply(x, k, s, _triple(padding))


# ----------------------------------------------------------------------------------------------- upsample


class _Upsample3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, out_size, mode, align_corners, ratios, out):
        _require_device(x)
        x, x_ld = _nd(x)
        n, c, d, h, w = x.shape
        do, ho, wo = out_size
        if out is None:
            y, y_ld = _new((n, c, do, ho, wo), x), c
        else:
            buf, y_off = out
            y_ld = _pitch_of(buf)
            if (y_ld != buf.shape[1] or tuple(buf.shape[2:]) != (do, ho, wo) or buf.shape[0] != n
                    or y_off + c > buf.shape[1] or buf.dtype != x.dtype):
                raise RuntimeError("upsample3d(out=): buffer %s cannot hold a %s slice at channel %d"
                                   % (tuple(buf.shape), (n, c, do, ho, wo), y_off))
            y = _slice_view(buf, y_off, c)
        g = UpGeom(n, d, h, w, do, ho, wo, c, x_ld, y_ld, mode, 1 if align_corners else 0, ratios[0], ratios[1], ratios[2],
                   _dt(x))
        _launch(_lib.lib().mri3d_upsample3d_fwd, lambda: "upsample_fwd c%d" % c,
                lambda: {"flops": 0.0, "bytes": _esz(x) * (x.numel() + y.numel())}, None, x.device, g, x, y)
        ctx.geom = g
        ctx.xshape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        dy, dy_ld = _nd(dy)
        dx = _new(ctx.xshape, dy)
        g = _repitched(ctx.geom, ctx.geom.c, dy_ld, _dt(dy))
        _launch(L.mri3d_upsample3d_bwd, lambda: "upsample_bwd c%d" % g.c, lambda: {"flops": 0.0, "bytes": _esz(dy) * (dx.numel() + dy.numel())},
                L.mri3d_upsample3d_workspace_bytes(ctypes.byref(g)), dy.device, g, dy, dx)
        return dx, None, None, None, None, None


def upsample3d(x, size=None, scale_factor=None, mode="nearest", align_corners=None, out=None):
    """torch.nn.functional.interpolate semantics for 5-D input, modes 'nearest' and 'trilinear'."""
    if mode == "linear":
        mode = "trilinear"
    if mode not in ("nearest", "trilinear"):
        raise NotImplementedError("upsample3d: mode %r is not supported" % (mode,))
    if mode == "nearest" and align_corners is not None:
        raise ValueError("align_corners option can only be set with the interpolating modes")
    in_sz = tuple(x.shape[2:])
    if (size is None) == (scale_factor is None):
        raise ValueError("exactly one of size or scale_factor must be given")
    if size is not None:
        out_sz = _triple(size)
        sf = None
    else:
        sf = tuple(float(s) for s in (scale_factor if isinstance(scale_factor, (tuple, list)) else (scale_factor,) * 3))
        out_sz = tuple(int(math.floor(float(i) * s)) for i, s in zip(in_sz, sf))
    ac = bool(align_corners)
    ratios = []
    for a in range(3):
        i, o = in_sz[a], out_sz[a]
        if mode == "trilinear" and ac:
            r = (i - 1) / (o - 1) if o > 1 else 0.0
        elif sf is not None:
            r = 1.0 / sf[a]          # torch uses the user-supplied scale when recompute_scale_factor is unset
        else:
            r = i / o
        ratios.append(float(r))
    code = UP_NEAREST if mode == "nearest" else UP_TRILINEAR
    return _Upsample3dFn.apply(x, out_sz, code, ac, tuple(ratios), out)


class _UpConv3dFn(torch.autograd.Function):
    """conv3d(upsample_nearest(x, scale), w, b, stride 1, padding) without the upsampled tensor (csrc/upconv.hip): the last
    UpBlock of the autoencoder (AE_model.py:110-120) — see upsample_conv3d."""

    @staticmethod
    def forward(ctx, x, weight, bias, scale, padding):
        _require_device(x)
        _require_param(weight, bias)
        x, x_ld = _nd(x)
        w = weight.contiguous()
        p = _upconv_passes(x.shape, w.shape, scale, padding, _dt(x), x_ld)
        g = p.fwd
        y = _new((g.n, g.co, g.dout, g.ho, g.wo), x)
        _launch(_lib.lib().mri3d_upconv3d_fwd, lambda: _conv_tag("fwd", g) + " of nearest x%d" % scale,
                lambda: {"flops": _conv_work(g, "fwd")["flops"], "bytes": _esz(x) * (x.numel() + y.numel())},
                None, None, g, scale, x, w, bias, y)
        ctx.save_for_backward(x, w)
        ctx.passes, ctx.scale, ctx.params = p, scale, (weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, w = ctx.saved_tensors
        scale = ctx.scale
        dy, y_ld = _nd(dy)
        p = _for_gradient_pitch(ctx.passes, y_ld)
        gd, gw = p.dgrad, p.wgrad
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _new(tuple(x.shape), x)
            _launch(L.mri3d_upconv3d_dgrad, lambda: _conv_tag("dgrad", gd) + " onto nearest x%d" % scale,
                    lambda: {"flops": _conv_work(gd, "dgrad")["flops"], "bytes": _esz(dy) * (dx.numel() + dy.numel())},
                    None, None, gd, scale, dy, w, dx)

        def wgrad(dw, db):
            _launch(L.mri3d_upconv3d_wgrad, lambda: _conv_tag("wgrad", gw) + " of nearest x%d" % scale,
                    lambda: {"flops": _conv_work(gw, "wgrad")["flops"], "bytes": _esz(dy) * (x.numel() + dy.numel())},
                    L.mri3d_upconv3d_workspace_bytes(ctypes.byref(gw), scale), x.device, gw, scale, x, dy, dw, db)
        return (dx, *_conv_param_grads(ctx, 1, ctx.params, wgrad), None, None)


def upsample_conv3d_supported(x, weight, scale, stride=1, padding=0, dilation=1):
    """True when conv3d(upsample_nearest(x, scale), weight) is served without the upsampled tensor (mri3d_upconv3d_supported)."""
    if not (isinstance(scale, int) or (isinstance(scale, float) and float(scale).is_integer())):
        return False
    scale = int(scale)
    if _triple(stride) != (1, 1, 1) or _triple(dilation) != (1, 1, 1) or x.dim() != 5 or not x.is_cuda:
        return False
    if x.data_ptr() % 16:      # a channel slice that does not start on four channels: the two operators take it
        return False
    if weight.shape[1] != x.shape[1]:
        return False
    try:
        g = _upconv_passes(tuple(x.shape), tuple(weight.shape), scale, _triple(padding), _dt(x), _pitch_of(x) or x.shape[1]).fwd
    except RuntimeError:
        return False
    return bool(_lib.lib().mri3d_upconv3d_supported(ctypes.byref(g), scale))


def upsample_conv3d(x, scale, weight, bias=None, padding=0):
    """conv3d(F.interpolate(x, scale_factor=scale, mode='nearest'), weight, bias, stride=1, padding=padding) — the head of the
    reference's UpBlock (AE_model.py:110-120) — through the fused operator where it is served, else through the two operators."""
    if upsample_conv3d_supported(x, weight, scale, 1, padding, 1):
        return _UpConv3dFn.apply(x, weight, bias, int(scale), _triple(padding))
    return conv3d(upsample3d(x, scale_factor=scale, mode="nearest"), weight, bias, stride=1, padding=padding)


# ----------------------------------------------------------------------------------------------- loss


# What a public loss function hands to `_ScalarLossFn`: the checked logits as the kernels read them (detached: the caller's tensor
# owns the gradient) and the C geometry, the length of `stats` and the workspace bytes, the fwd / bwd entry names, the pointer
# arguments between the logits and the loss (target, labels, weights, a map: tensors or None) and what the backward passes
# after the gradient (a pitch).
_LossRecord = collections.namedtuple("_LossRecord", "logits geom stats_len ws_bytes fwd bwd extra bwd_tail", defaults=((),))


class _ScalarLossFn(torch.autograd.Function):
    """A scalar loss of logits: fwd(g, logits, *extra, loss, stats, workspace, bytes, stream) leaves the loss and the `stats` that
    bwd(g, logits, *extra, stats, dloss, dlogits, *bwd_tail, stream) turns into the dense gradient.  `logits` is the caller's
    tensor (the gradient's owner); the kernels read rec.logits."""

    @staticmethod
    def forward(ctx, logits, rec):
        x = rec.logits
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        stats = torch.empty(rec.stats_len, dtype=torch.float32, device=x.device)
        ws = _workspace(rec.ws_bytes, x.device)
        check(getattr(_lib.lib(), rec.fwd)(ctypes.byref(rec.geom), _ptr(x), *map(_ptr, rec.extra), _ptr(loss), _ptr(stats), _ptr(ws),
                                           ws.numel(), _stream()), rec.fwd[len("mri3d_"):])
        ctx.save_for_backward(x, stats, *rec.extra)
        ctx.rec = rec
        return loss

    @staticmethod
    def backward(ctx, dloss):
        x, stats, *extra = ctx.saved_tensors
        rec = ctx.rec
        dloss = dloss.to(torch.float32).contiguous()
        dlogits = _new(x.shape, x)
        check(getattr(_lib.lib(), rec.bwd)(ctypes.byref(rec.geom), _ptr(x), *map(_ptr, extra), _ptr(stats), _ptr(dloss), _ptr(dlogits),
                                           *rec.bwd_tail, _stream()), rec.bwd[len("mri3d_"):])
        return dlogits, None


def softmax_dice_loss(logits, target, eps=1e-9):
    """mean over (n, c) of 1 - dice(softmax(logits)[:, c], target) — segmentation/routine.py:272-274 in one kernel."""
    target = target.to(torch.float32)
    _require_device(logits)
    _require_param(target)
    x, target = _cl(logits.detach()), _cl(target.detach())
    n, c, d, h, w = x.shape
    ct = target.shape[1]
    if tuple(target.shape) != (n, ct, d, h, w) or ct not in (1, c):
        raise RuntimeError("softmax_dice_loss: target shape %s incompatible with logits %s"
                           % (tuple(target.shape), tuple(x.shape)))
    g = DiceGeom(n, d * h * w, c, ct, c, ct, float(eps), _dt(x))
    return _ScalarLossFn.apply(logits, _LossRecord(x, g, n * c * 3, _lib.lib().mri3d_softmax_dice_workspace_bytes(ctypes.byref(g)),
                                            "mri3d_softmax_dice_fwd", "mri3d_softmax_dice_bwd", (target,)))


def argmax_mask(logits):
    """logits.argmax(dim=1) as a uint8 (N, D, H, W) mask — segmentation/routine.py:226-227."""
    _require_device(logits)
    L = _lib.lib()
    logits = _cl(logits.detach())
    n, c, d, h, w = logits.shape
    out = torch.empty((n, d, h, w), dtype=torch.uint8, device=logits.device)
    check(L.mri3d_argmax_u8(_ptr(logits), _ptr(out), n * d * h * w, c, c, _dt(logits), _stream()), "argmax_u8")
    return out


# Monte-Carlo predictive statistics (csrc/mc_stats.hip): T sampled forward passes -> mean prediction + uncertainty maps
MC_OUTPUTS = ("mean", "variance", "entropy", "mutual_info", "mask")


def _mc_dims(shape):
    if len(shape) != 5:
        raise RuntimeError("expected a 5-D (N,C,D,H,W) logits shape, got %s" % (tuple(shape),))
    n, c, d, h, w = (int(s) for s in shape)
    return n, c, d, h, w, n * d * h * w


def mc_state(logits_shape, device):
    """The accumulator of `mc_accumulate` for logits of logical shape (N, C, D, H, W): an opaque float32 tensor sized by
    mri3d_mc_state_bytes.  It need not be cleared: the first `mc_accumulate(..., first=True)` overwrites it."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("mc_state: the Monte-Carlo statistics run only on a ROCm device (got %s); there is no CPU fallback" % device)
    n, c, d, h, w, nvox = _mc_dims(logits_shape)
    nbytes = _lib.lib().mri3d_mc_state_bytes(nvox, c)
    if nbytes == 0:
        raise RuntimeError("mc_state: unsupported logits shape %s (needs 2..32 classes and at least one voxel)" % (tuple(logits_shape),))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def mc_accumulate(state, logits, first, reps=1):
    """Add `reps` stacked draws to `state`: `logits` is (reps*N, C, D, H, W) as the models return it (fp32 or bf16), draw r of
    volume n at batch index r*N + n; softmax, p, p^2 and p log p per draw in one read-modify-write of the state.
    first=True overwrites the state instead of adding to it."""
    _require_device(logits)
    _require_param(state)
    if reps < 1 or logits.shape[0] % reps:
        raise RuntimeError("mc_accumulate: batch %d is not %d stacked draws" % (logits.shape[0], reps))
    L = _lib.lib()
    logits, ld = _nd(logits.detach())
    n, c, d, h, w, total = _mc_dims(logits.shape)
    nvox = total // reps
    check(L.mri3d_mc_accumulate(_ptr(logits), nvox, c, ld, _dt(logits), reps, nvox, 1 if first else 0, _ptr(state),
                                state.numel() * 4, _stream()), "mc_accumulate")


def mc_finalize(state, shape, samples, want=MC_OUTPUTS):
    """Read `state` out after `samples` draws of logits of logical shape `shape` = (N, C, D, H, W).  Returns a dict with the
    entries named in `want`: "mean" and "variance" (N, C, D, H, W) float32 in channels-last storage, "entropy" and "mutual_info"
    (N, D, H, W) float32, "mask" (N, D, H, W) uint8 = arg-max of the mean (first maximum).
    `shape` must be the shape the state was made and filled for: the state records no shape, so only its size is checked (it
    must be exactly `mc_state(shape)`'s), and a permuted shape with the same voxel and class counts would relabel the maps
    silently.  `MCAccumulator` keeps the two together."""
    _require_param(state)
    want = tuple(want)
    if not want or any(k not in MC_OUTPUTS for k in want):
        raise RuntimeError("mc_finalize: want must name some of %s, got %s" % (MC_OUTPUTS, want))
    L = _lib.lib()
    n, c, d, h, w, nvox = _mc_dims(shape)
    if state.numel() * 4 != L.mri3d_mc_state_bytes(nvox, c):
        raise RuntimeError("mc_finalize: a state of %d floats is not the state of logits of shape %s" % (state.numel(), tuple(shape)))
    out = {}
    for k in MC_OUTPUTS:
        if k not in want:
            out[k] = None
        elif k in ("mean", "variance"):
            out[k] = torch.empty((n, c, d, h, w), dtype=torch.float32, device=state.device, memory_format=CL3D)
        else:
            out[k] = torch.empty((n, d, h, w), dtype=torch.uint8 if k == "mask" else torch.float32, device=state.device)
    check(L.mri3d_mc_finalize(_ptr(state), state.numel() * 4, nvox, c, int(samples), *(_ptr(out[k]) for k in MC_OUTPUTS),
                              _stream()), "mc_finalize")
    return {k: out[k] for k in want}


def _require_labels(who, *ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("%s runs only on ROCm device tensors (got %s); there is no CPU fallback" % (who, t.device))


def _u8_pair(who, what, pred, gt):
    """Two uint8 device maps of one shape, contiguous."""
    for t in (pred, gt):
        _require_labels(who, t)
        if t.dtype != torch.uint8:
            raise RuntimeError("%s: %s must be uint8, got %s" % (who, what, t.dtype))
    if pred.shape != gt.shape:
        raise RuntimeError("%s: shapes differ %s vs %s" % (who, tuple(pred.shape), tuple(gt.shape)))
    return pred.contiguous(), gt.contiguous()


def mask_overlap_counts(pred, gt):
    """Exact overlap counts of two uint8 masks on the device -> int64 tensor
    [sum(gt), sum(pred), sum(gt & pred), #(gt>0 & pred>0), #(gt>0 | pred>0)]  (validate_dsc_asd's Dice / IoU inputs,
    segmentation/routine.py:198-235, metrics.py:312-329)."""
    pred, gt = _u8_pair("mask_overlap_counts", "masks", pred, gt)
    L = _lib.lib()
    out = torch.empty(5, dtype=torch.int64, device=pred.device)
    ws = _workspace(L.mri3d_mask_overlap_workspace_bytes(), pred.device)
    check(L.mri3d_mask_overlap(_ptr(pred), _ptr(gt), pred.numel(), _ptr(out), _ptr(ws), ws.numel(), _stream()),
          "mask_overlap")
    return out


def dice_iou_from_counts(counts):
    """(Dice, IoU) floats with the reference's arithmetic: 2*|gt&pred| / (|gt|+|pred|), NaN if both masks are empty
    (metrics.py:323-329); intersection / union as Python floats (routine.py:198-203; ZeroDivisionError if both empty)."""
    import numpy as np
    sg, sp, sand, n_and, n_or = (int(v) for v in counts.tolist())
    dsc = float("nan") if sg + sp == 0 else 2 * sand / (sg + sp)
    # the reference sums float32 indicator arrays and divides `float(intersection) / union` with union an np.float32:
    # the same expression on the (exactly representable up to 2^24 voxels) counts
    intersection, union = np.float32(n_and), np.float32(n_or)
    return dsc, float(intersection) / union


# ----------------------------------------------------------------------------------------------- label maps (csrc/labels.hip)
_LABEL_DTYPES = {torch.uint8: _lib.LABEL_U8, torch.int16: _lib.LABEL_I16, torch.int32: _lib.LABEL_I32,
                 torch.float32: _lib.LABEL_F32}


def remap_labels(labels, lut, above=0, other=0, out_dtype=torch.uint8, out=None):
    """Raw label ids -> classes through a uint8 device table: v >= len(lut) -> `above`, v an integer in [0, len(lut)) -> lut[v],
    anything else (negative, fractional, NaN) -> `other`.  `labels` is uint8 / int16 / int32 / float32 of any shape, the result
    uint8 or float32 of that shape; out=labels (same dtype) remaps in place.  prepare_batch's binarisation
    (segmentation/routine.py:185-196) is one table of this kind, a parcellation's class map another (segmentation/labels.py)."""
    _require_labels("remap_labels", labels, lut)
    if labels.dtype not in _LABEL_DTYPES:
        raise RuntimeError("remap_labels: labels must be uint8, int16, int32 or float32, got %s" % labels.dtype)
    if lut.dtype != torch.uint8 or lut.dim() != 1 or not lut.is_contiguous():
        raise RuntimeError("remap_labels: the table must be a contiguous 1-D uint8 tensor")
    if out is None:
        if out_dtype not in (torch.uint8, torch.float32):
            raise RuntimeError("remap_labels: out_dtype must be uint8 or float32, got %s" % out_dtype)
        out = torch.empty(labels.shape, dtype=out_dtype, device=labels.device)
        labels = labels.contiguous()
    elif out.shape != labels.shape or not out.is_contiguous() or not labels.is_contiguous() or out.device != labels.device \
            or out.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError("remap_labels: out must be a contiguous uint8 / float32 tensor of the (contiguous) labels' shape and device")
    if labels.numel():
        check(_lib.lib().mri3d_label_remap(_ptr(labels), _LABEL_DTYPES[labels.dtype], _ptr(out), _LABEL_DTYPES[out.dtype],
                                           labels.numel(), _ptr(lut), lut.numel(), int(above), int(other), _stream()), "label_remap")
    return out


def _class_map(who, logits, labels):
    """The uint8 class map `labels` (N, 1, D, H, W) or (N, D, H, W) of `logits`, checked: (dense NDHWC logits, contiguous labels, n,
    voxels of a sample, classes)."""
    _require_device(logits)
    _require_labels(who, labels)
    if labels.dtype != torch.uint8:
        raise RuntimeError("%s: labels must be a uint8 class map, got %s" % (who, labels.dtype))
    x = _cl(logits.detach())
    n, c, d, h, w = x.shape
    if tuple(labels.shape) not in ((n, 1, d, h, w), (n, d, h, w)):
        raise RuntimeError("%s: labels shape %s incompatible with logits %s" % (who, tuple(labels.shape), tuple(x.shape)))
    return x, labels.contiguous(), n, d * h * w, c


def softmax_dice_index_loss(logits, labels, eps=1e-9):
    """`softmax_dice_loss` with the target as a uint8 class map (N, 1, D, H, W) or (N, D, H, W) instead of float one-hot channels:
    mean over (n, c) of 1 - dice(softmax(logits)[:, c], labels == c), for 2..32 classes.  A label >= C belongs to no class (the
    voxel is ignored by every class's numerator and target sum).  One byte of target per voxel instead of 4*C.  It launches by the
    plan that `ce_index_plan` reports: one function of the library decides for the whole class-map family."""
    x, labels, n, vox, c = _class_map("softmax_dice_index_loss", logits, labels)
    g = _lib.DiceIndexGeom(n, vox, c, c, float(eps), _dt(x))
    return _ScalarLossFn.apply(logits, _LossRecord(x, g, n * c * 3, _lib.lib().mri3d_softmax_dice_index_workspace_bytes(ctypes.byref(g)),
                                            "mri3d_softmax_dice_index_fwd", "mri3d_softmax_dice_index_bwd", (labels,)))


# ----------------------------------------------------------------------------------------------- cross-entropy / focal (csrc/ce_loss.hip)
CE_PLAN_FIELDS = tuple(f for f, _ in _lib.CeIndexPlanInfo._fields_)
CE_READ_MODES = {0: "scalar", 1: "rows4", 2: "vox4"}


def _ce_settings(who, gamma, dice_weight, ce_weight):
    """The scalar settings of the CE family as floats; what the library would refuse is refused here by name."""
    gamma, dice_weight, ce_weight = float(gamma), float(dice_weight), float(ce_weight)
    if not (gamma == 0.0 or 1.0 <= gamma <= 8.0):
        raise RuntimeError("%s: gamma must be 0 or in [1, 8], got %r" % (who, gamma))
    if not (0.0 <= dice_weight < float("inf") and 0.0 <= ce_weight < float("inf")) or dice_weight + ce_weight == 0.0:
        raise RuntimeError("%s: dice_weight and ce_weight must be finite, not negative and not both zero, got %r and %r"
                           % (who, dice_weight, ce_weight))
    return gamma, dice_weight, ce_weight


def ce_index_plan(n, vox, c, dtype=torch.float32, pass_=_lib.PASS_FWD, x_ld=None, dice_weight=0.0, ce_weight=1.0, gamma=0.0,
                  align_logits=16, align_labels=16):
    """What `softmax_ce_index_loss` / `softmax_dice_ce_index_loss` and `softmax_dice_index_loss` launch by for `n` samples of `vox` voxels and `c` classes, host
    only: a dict of CE_PLAN_FIELDS (Mri3dCeIndexPlanInfo, include/mri3d.h) with the read mode by name.  pass_: _lib.PASS_FWD or
    _lib.PASS_DGRAD (the backward); align_*: the largest power of two <= 16 dividing the addresses."""
    g = _lib.CeIndexGeom(int(n), int(vox), int(c), int(c if x_ld is None else x_ld), 1e-9, BF16 if dtype == torch.bfloat16 else F32,
                         float(gamma), float(dice_weight), float(ce_weight))
    info = _lib.CeIndexPlanInfo()
    check(_lib.lib().mri3d_softmax_ce_index_plan_query(ctypes.byref(g), int(pass_), int(align_logits), int(align_labels),
                                                       ctypes.byref(info)), "softmax_ce_index_plan_query")
    out = {f: getattr(info, f) for f in CE_PLAN_FIELDS}
    out["mode"] = CE_READ_MODES[out["mode"]]
    return out


def _ce_loss(who, logits, labels, weight, gamma, dice_weight, ce_weight, eps):
    """dice_weight * Dice_index + ce_weight * CE in one forward and one backward pass (dice_weight == 0: the CE-only kernels)."""
    x, labels, n, vox, c = _class_map(who, logits, labels)
    gamma, dice_weight, ce_weight = _ce_settings(who, gamma, dice_weight, ce_weight)
    if weight is not None:
        if not torch.is_tensor(weight) or weight.device != x.device or weight.dtype != torch.float32 \
                or tuple(weight.shape) != (c,):
            raise RuntimeError("%s: weight must be a float32 tensor of %d entries on %s, got %s"
                               % (who, c, x.device, "%s %s on %s" % (weight.dtype, tuple(weight.shape), weight.device)
                                  if torch.is_tensor(weight) else type(weight).__name__))
        weight = weight.detach().contiguous()
    g = _lib.CeIndexGeom(n, vox, c, c, float(eps), _dt(x), gamma, dice_weight, ce_weight)
    return _ScalarLossFn.apply(logits, _LossRecord(x, g, 4 + n * c * 3, _lib.lib().mri3d_softmax_ce_index_workspace_bytes(ctypes.byref(g)),
                                            "mri3d_softmax_ce_index_fwd", "mri3d_softmax_ce_index_bwd", (labels, weight)))


def softmax_ce_index_loss(logits, labels, weight=None, gamma=0.0):
    """Voxel-wise cross-entropy (gamma = 0) or focal loss (gamma in [1, 8]) of softmax(logits) against a uint8 class map
    (N, 1, D, H, W) or (N, D, H, W), 2..32 classes:  sum_v -w_y (1 - p_y)^gamma log p_y / sum_v w_y over the voxels of the whole batch
    whose label is a class; a label >= C marks an ignored voxel.  `weight`: float32 device tensor of C class weights, or None for
    ones.  gamma = 0 is F.cross_entropy(logits, labels, weight, ignore_index, reduction="mean") — except that when no voxel counts
    (everything ignored, or every class that occurs has weight 0) the loss is 0 and its gradient exactly 0 where torch gives NaN:
    a patch outside the labelled region must not poison a run.  Device tensors only; there is no CPU fallback."""
    return _ce_loss("softmax_ce_index_loss", logits, labels, weight, gamma, 0.0, 1.0, 1e-9)


def softmax_dice_ce_index_loss(logits, labels, dice_weight=1.0, ce_weight=1.0, weight=None, gamma=0.0, eps=1e-9):
    """dice_weight * softmax_dice_index_loss(logits, labels, eps) + ce_weight * softmax_ce_index_loss(logits, labels, weight, gamma),
    each pass reading the logits once: the bytes of the index Dice alone.  The CE term is 0 with a zero gradient when no voxel
    counts (see softmax_ce_index_loss); the class weights apply to the CE term only."""
    return _ce_loss("softmax_dice_ce_index_loss", logits, labels, weight, gamma, dice_weight, ce_weight, eps)


def confusion_counts(pred, gt, classes):
    """Exact confusion counts of two uint8 class maps on the device: (conf, outside) with conf[g, p] = #(gt == g and pred == p), an
    int64 (C, C) device tensor, and outside = #(gt >= C or pred >= C), an int64 device scalar.  2 <= classes <= 32."""
    pred, gt = _u8_pair("confusion_counts", "class maps", pred, gt)
    L = _lib.lib()
    c = int(classes)
    out = torch.empty(max(c, 0) * max(c, 0) + 1, dtype=torch.int64, device=pred.device)
    ws = _workspace(L.mri3d_confusion_workspace_bytes(c), pred.device)
    check(L.mri3d_confusion_counts(_ptr(pred), _ptr(gt), pred.numel(), c, _ptr(out), _ptr(ws), ws.numel(), _stream()),
          "confusion_counts")
    return out[:c * c].view(c, c), out[c * c]


def class_scores_from_confusion(conf):
    """Per-class (Dice, IoU) float64 arrays of a (C, C) confusion matrix conf[gt, pred], each class scored as the binary mask
    `== c` with `dice_iou_from_counts`' arithmetic: 2*tp / (|gt| + |pred|) and float32(tp) / float32(|gt or pred|); NaN where the
    denominator is 0."""
    import numpy as np
    m = conf.cpu().numpy() if torch.is_tensor(conf) else np.asarray(conf)
    m = m.astype(np.int64)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise RuntimeError("class_scores_from_confusion: expected a square matrix, got shape %s" % (m.shape,))
    dice, iou = np.full(m.shape[0], np.nan), np.full(m.shape[0], np.nan)
    for k in range(m.shape[0]):
        tp, sg, sp = int(m[k, k]), int(m[k, :].sum()), int(m[:, k].sum())
        if sg + sp:
            dice[k] = 2 * tp / (sg + sp)
            iou[k] = float(np.float32(tp)) / np.float32(sg + sp - tp)
    return dice, iou


# ----------------------------------------------------------------------------------------------- connected components (csrc/components.hip)
COMPONENTS_PLAN_FIELDS = tuple(f for f, _ in _lib.ComponentsPlanInfo._fields_)
COMPONENT_STATS_COLUMNS = ("count", "overlap", "dmin", "dmax", "hmin", "hmax", "wmin", "wmax")
_CONNECTIVITY = {1: 6, 2: 18, 3: 26, 6: 6, 18: 18, 26: 26}


def _connectivity(who, connectivity):
    if connectivity not in _CONNECTIVITY:
        raise ValueError("%s: connectivity must be 6, 18 or 26 (or scipy's 1, 2, 3), got %r" % (who, connectivity))
    return _CONNECTIVITY[connectivity]


def _dhw(who, t):
    """A (d, h, w) volume or an (h, w) map (d = 1) as its three extents."""
    if t.dim() not in (2, 3):
        raise RuntimeError("%s: expected a (d, h, w) volume or an (h, w) map, got shape %s" % (who, tuple(t.shape)))
    return (1,) * (3 - t.dim()) + tuple(int(s) for s in t.shape)


def _volume_like(who, what, t, dtype, like):
    """An optional companion volume of `like`'s shape and device, contiguous, of the given dtype (bool counts as uint8)."""
    if t is None:
        return None
    _require_labels(who, t)
    if t.dtype == torch.bool and dtype == torch.uint8:
        t = t.view(torch.uint8)
    if t.dtype != dtype or t.shape != like.shape or t.device != like.device:
        raise RuntimeError("%s: %s must be a %s tensor of shape %s on %s, got %s %s on %s"
                           % (who, what, dtype, tuple(like.shape), like.device, t.dtype, tuple(t.shape), t.device))
    return t.contiguous()


def components_plan(shape, connectivity):
    """What the launches of `label_components` go by for a (d, h, w) or (h, w) shape: COMPONENTS_PLAN_FIELDS as a dict (host only)."""
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3):
        raise RuntimeError("components_plan: expected (d, h, w) or (h, w), got %s" % (shape,))
    d, h, w = (1,) * (3 - len(shape)) + shape
    info = _lib.ComponentsPlanInfo()
    rc = _lib.lib().mri3d_components_plan_query(d, h, w, _connectivity("components_plan", connectivity), ctypes.byref(info))
    if rc != 0:
        raise RuntimeError("components_plan: the library refuses shape %s (rc=%d)" % (shape, rc))
    return {f: getattr(info, f) for f in COMPONENTS_PLAN_FIELDS}


def label_components(mask, connectivity=6, by_value=False, out=None):
    """Connected components of a uint8 / bool device mask (d, h, w) or (h, w) -> (labels, count): int32 labels of the mask's
    shape, 0 for background and 1..K numbered by each component's first voxel in C order (scipy.ndimage.label's numbering, the
    same bits every run), and K as an int32 device scalar.  connectivity 6 / 18 / 26 (or scipy's 1 / 2 / 3); by_value: voxels
    connect only when their values are equal and non-zero (the components of every class of a class map)."""
    who = "label_components"
    _require_labels(who, mask)
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8:
        raise RuntimeError("%s: the mask must be uint8 or bool, got %s" % (who, mask.dtype))
    conn = _connectivity(who, connectivity)
    d, h, w = _dhw(who, mask)
    mask = mask.contiguous()
    if out is None:
        out = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    elif out.dtype != torch.int32 or out.shape != mask.shape or out.device != mask.device or not out.is_contiguous():
        raise RuntimeError("%s: out must be a contiguous int32 tensor of the mask's shape and device" % who)
    count = torch.zeros((), dtype=torch.int32, device=mask.device)
    if mask.numel():
        L = _lib.lib()
        ws = _workspace(L.mri3d_components_workspace_bytes(d, h, w), mask.device)
        check(L.mri3d_components_label(_ptr(mask), d, h, w, conn, int(bool(by_value)), _ptr(out), _ptr(count), _ptr(ws), ws.numel(),
                                       _stream()), "components_label")
    return out, count


def component_stats(labels, capacity, other=None, other_labels=None, score=None, other_capacity=None, out=None):
    """Per-component tables of an int32 label volume, ids 1..capacity (row id - 1; ids above are dropped), as device tensors:
      "stats"  int64 (capacity, 8), columns COMPONENT_STATS_COLUMNS: voxels, voxels with other != 0 (`other`: a uint8 / bool mask),
               and the inclusive bounding box; a row no voxel reaches holds 0, 0, d, -1, h, -1, w, -1
      "peak"   float32 (capacity,), the maximum of the float32 volume `score` over the component (with `score`; finite scores)
      "hit"    uint8 (other_capacity,), 1 where component j + 1 of the int32 volume `other_labels` shares a voxel with any labelled
               voxel of `labels` (with `other_labels`; other_capacity is then required)
    out: a dict of preallocated contiguous tensors for any of the three."""
    who = "component_stats"
    _require_labels(who, labels)
    if labels.dtype != torch.int32:
        raise RuntimeError("%s: labels must be int32, got %s" % (who, labels.dtype))
    d, h, w = _dhw(who, labels)
    labels = labels.contiguous()
    capacity = int(capacity)
    if capacity <= 0:
        raise ValueError("%s: capacity must be positive, got %d" % (who, capacity))
    other = _volume_like(who, "other", other, torch.uint8, labels)
    score = _volume_like(who, "score", score, torch.float32, labels)
    other_labels = _volume_like(who, "other_labels", other_labels, torch.int32, labels)
    if (other_labels is None) != (other_capacity is None) or (other_capacity is not None and int(other_capacity) <= 0):
        raise ValueError("%s: other_labels and a positive other_capacity are given together" % who)
    out = {} if out is None else out
    want = {"stats": ((capacity, 8), torch.int64)}
    if score is not None:
        want["peak"] = ((capacity,), torch.float32)
    if other_labels is not None:
        want["hit"] = ((int(other_capacity),), torch.uint8)
    res = {}
    for k, (shape, dtype) in want.items():
        t = out.get(k)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=labels.device)
        elif tuple(t.shape) != shape or t.dtype != dtype or t.device != labels.device or not t.is_contiguous():
            raise RuntimeError("%s: out[%r] must be a contiguous %s tensor of shape %s on the labels' device" % (who, k, dtype, shape))
        res[k] = t
    if labels.numel() == 0:
        raise RuntimeError("%s: empty volume" % who)
    check(_lib.lib().mri3d_components_stats(_ptr(labels), d, h, w, capacity, _ptr(other), _ptr(score), _ptr(res["stats"]),
                                            _ptr(res.get("peak")), _ptr(other_labels), int(other_capacity or 0), _ptr(res.get("hit")),
                                            _stream()), "components_stats")
    return res


def select_components(labels, keep, out=None):
    """out[i] = keep[labels[i]]: the uint8 mask of the components a uint8 device table keeps (count + 1 entries, keep[0] = 0 for
    the background; a label beyond the table selects 0).  One streaming pass."""
    who = "select_components"
    _require_labels(who, labels, keep)
    if labels.dtype != torch.int32:
        raise RuntimeError("%s: labels must be int32, got %s" % (who, labels.dtype))
    if keep.dtype == torch.bool:
        keep = keep.view(torch.uint8)
    if keep.dtype != torch.uint8 or keep.dim() != 1 or keep.numel() == 0 or keep.device != labels.device:
        raise RuntimeError("%s: keep must be a non-empty 1-D uint8 / bool tensor on the labels' device" % who)
    labels, keep = labels.contiguous(), keep.contiguous()
    if out is None:
        out = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
    elif out.dtype != torch.uint8 or out.shape != labels.shape or out.device != labels.device or not out.is_contiguous():
        raise RuntimeError("%s: out must be a contiguous uint8 tensor of the labels' shape and device" % who)
    if labels.numel():
        check(_lib.lib().mri3d_components_select(_ptr(labels), labels.numel(), _ptr(keep), keep.numel(), _ptr(out), _stream()),
              "components_select")
    return out


# ----------------------------------------------------------------------------------------------- distance maps (csrc/distance.hip)
EDT_PLAN_FIELDS = tuple(f for f, _ in _lib.EdtPlanInfo._fields_)
EDT_INF = _lib.EDT_INF
INT32_MIN = -2 ** 31


def _batch_dhw(who, t):
    """A (d, h, w) volume, an (h, w) map (d = 1) or a batch (n, d, h, w) as (n, d, h, w)."""
    if t.dim() not in (2, 3, 4):
        raise RuntimeError("%s: expected (h, w), (d, h, w) or (n, d, h, w), got shape %s" % (who, tuple(t.shape)))
    return (1,) * (4 - t.dim()) + tuple(int(s) for s in t.shape)


def _u8_volume(who, t):
    _require_labels(who, t)
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise RuntimeError("%s: expected a uint8 or bool tensor, got %s" % (who, t.dtype))
    if t.numel() == 0:
        raise RuntimeError("%s: empty volume" % who)
    return t.contiguous()


def _out_like(who, out, shape, dtype, like):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or out.device != like.device or not out.is_contiguous():
        raise RuntimeError("%s: out must be a contiguous %s tensor of shape %s on the input's device" % (who, dtype, tuple(shape)))
    return out


def _edt_value(who, value):
    if value is None:
        return -1
    if not 0 <= int(value) <= 255:
        raise ValueError("%s: value must be None or a byte, got %r" % (who, value))
    return int(value)


def edt_plan(shape):
    """What the three passes of the distance transform launch by for an (n, d, h, w), (d, h, w) or (h, w) shape: EDT_PLAN_FIELDS as
    a dict (Mri3dEdtPlanInfo, include/mri3d.h).  Host only."""
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3, 4):
        raise RuntimeError("edt_plan: expected (h, w), (d, h, w) or (n, d, h, w), got %s" % (shape,))
    n, d, h, w = (1,) * (4 - len(shape)) + shape
    info = _lib.EdtPlanInfo()
    rc = _lib.lib().mri3d_edt_plan(n, d, h, w, ctypes.byref(info))
    if rc != 0:
        raise RuntimeError("edt_plan: the library refuses shape %s (rc=%d)" % (shape, rc))
    return {f: getattr(info, f) for f in EDT_PLAN_FIELDS}


def edt_sq(mask, value=None, outside_zero=False, out=None):
    """Exact squared Euclidean distance transform of a uint8 / bool device tensor (h, w), (d, h, w) or a batch (n, d, h, w): int32
    of the same shape, the squared distance in voxels to the nearest zero voxel of the same volume (scipy's
    distance_transform_edt, squared, bit for bit).  value: a voxel is inside when it equals `value` instead of when it is non-zero.
    outside_zero: the volume is surrounded by zeros.  A volume without a zero voxel gives EDT_INF everywhere."""
    who = "edt_sq"
    mask = _u8_volume(who, mask)
    n, d, h, w = _batch_dhw(who, mask)
    out = _out_like(who, out, mask.shape, torch.int32, mask)
    L = _lib.lib()
    ws = _workspace(L.mri3d_edt_workspace_bytes(n, d, h, w), mask.device)
    check(L.mri3d_edt_sq_u8(_ptr(mask), n, d, h, w, _edt_value(who, value), int(bool(outside_zero)), _ptr(out), _ptr(ws), ws.numel(),
                            _stream()), "edt_sq_u8")
    return out


def edt_threshold(mask, r2, greater=False, value=None, outside_zero=False, out=None):
    """uint8 (edt_sq(mask, value, outside_zero) <= r2), or (> r2) with greater, in the transform's last pass: the int32 map is never
    written.  r2 is an integer >= 0 (above EDT_INF - 1 it is EDT_INF - 1: a saturated volume is further than any radius)."""
    who = "edt_threshold"
    mask = _u8_volume(who, mask)
    n, d, h, w = _batch_dhw(who, mask)
    out = _out_like(who, out, mask.shape, torch.uint8, mask)
    if int(r2) < 0:
        raise ValueError("%s: r2 must not be negative, got %r" % (who, r2))
    L = _lib.lib()
    ws = _workspace(L.mri3d_edt_workspace_bytes(n, d, h, w), mask.device)
    check(L.mri3d_edt_threshold_u8(_ptr(mask), n, d, h, w, _edt_value(who, value), int(bool(outside_zero)), min(int(r2), EDT_INF - 1),
                                   int(bool(greater)), _ptr(out), _ptr(ws), ws.numel(), _stream()), "edt_threshold_u8")
    return out


def _class_ids(who, classes, ids):
    classes, ids = int(classes), tuple(int(i) for i in ids)
    if not 2 <= classes <= 32:
        raise ValueError("%s: classes must be in [2, 32], got %d" % (who, classes))
    if not 1 <= len(ids) <= 32 or any(not 0 <= i < classes for i in ids) or len(set(ids)) != len(ids):
        raise ValueError("%s: ids are 1 to 32 distinct classes below %d, got %r" % (who, classes, ids))
    return classes, ids


def signed_sqdist(class_map, classes, ids, out=None):
    """Signed squared-distance maps of a uint8 device class map (n, d, h, w) or (n, 1, d, h, w): int32 (n, K, d, h, w), one plane per
    class id.  INT32_MIN at a voxel whose label is >= classes; 0 everywhere in a volume the class is absent from or fills; + the
    squared distance to the class outside it; - the squared distance to what is not the class inside it.  Nothing comes to the host:
    the call can stand inside a captured step."""
    who = "signed_sqdist"
    classes, ids = _class_ids(who, classes, ids)
    class_map = _u8_volume(who, class_map)
    if class_map.dim() == 5 and class_map.shape[1] == 1:
        class_map = class_map[:, 0]
    if class_map.dim() != 4:
        raise RuntimeError("%s: expected a class map (n, d, h, w) or (n, 1, d, h, w), got shape %s" % (who, tuple(class_map.shape)))
    n, d, h, w = (int(s) for s in class_map.shape)
    out = _out_like(who, out, (n, len(ids), d, h, w), torch.int32, class_map)
    L = _lib.lib()
    ws = _workspace(L.mri3d_edt_workspace_bytes(n, d, h, w), class_map.device)
    check(L.mri3d_signed_sqdist_u8(_ptr(class_map), n, d, h, w, classes, (ctypes.c_int32 * len(ids))(*ids), len(ids), _ptr(out), _ptr(ws),
                                   ws.numel(), _stream()), "signed_sqdist_u8")
    return out


def softmax_boundary_loss(logits, signed_map, ids):
    """Boundary loss (Kervadec et al., MIDL 2019): the mean over classes `ids` and voxels of softmax(logits)[:, id] * phi(s), with s
    the int32 map of `signed_sqdist(class_map, C, ids)` and phi(s) = sqrt(s), -(sqrt(-s) - 1) or 0 for s > 0, < 0, = 0.  Terms with
    s == INT32_MIN (ignored voxels) are left out of the sum and of the count; with none left the loss is 0 and its gradient zero.
    logits: fp32 / bf16 (n, C, d, h, w), NDHWC with any voxel pitch, 2..32 classes.  No gradient flows into the map."""
    who = "softmax_boundary_loss"
    _require_device(logits)
    _require_labels(who, signed_map)
    x, x_ld = _nd(logits.detach())                # the logits keep their voxel pitch; the gradient is dense
    n, c, d, h, w = x.shape
    _, ids = _class_ids(who, c, ids)
    if signed_map.dtype != torch.int32 or tuple(signed_map.shape) != (n, len(ids), d, h, w) or signed_map.device != x.device:
        raise RuntimeError("%s: the map must be int32 of shape %s on %s, got %s %s on %s"
                           % (who, (n, len(ids), d, h, w), x.device, signed_map.dtype, tuple(signed_map.shape), signed_map.device))
    g = _lib.BoundaryGeom(n, d * h * w, c, x_ld, _dt(x), len(ids), (ctypes.c_int32 * 32)(*ids))
    return _ScalarLossFn.apply(logits, _LossRecord(x, g, 4, _lib.lib().mri3d_softmax_boundary_workspace_bytes(), "mri3d_softmax_boundary_fwd",
                                            "mri3d_softmax_boundary_bwd", (signed_map.detach().contiguous(),), (c,)))


# ----------------------------------------------------------------------------------------------- intensity statistics (csrc/intensity.hip)
def _intensity_rows(who, x, mask):
    """x as (B, n) float32 rows (a 1-D tensor is one row, anything else a batch along its first axis) and the matching mask rows."""
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError("%s: needs a float32 ROCm device tensor (got %s on %s); there is no CPU fallback" % (who, x.dtype, x.device))
    rows = x.contiguous().reshape(1, -1) if x.dim() <= 1 else x.contiguous().reshape(x.shape[0], -1)
    if rows.shape[0] == 0 or rows.shape[1] == 0:
        raise RuntimeError("%s: empty tensor of shape %s" % (who, tuple(x.shape)))
    if mask is not None:
        if not mask.is_cuda or mask.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError("%s: the mask must be a bool / uint8 ROCm device tensor (got %s on %s); there is no CPU fallback"
                               % (who, mask.dtype, mask.device))
        if mask.numel() != rows.numel():
            raise RuntimeError("%s: mask of shape %s does not match the tensor's %s" % (who, tuple(mask.shape), tuple(x.shape)))
        mask = mask.contiguous().view(torch.uint8).reshape(rows.shape)
    return rows, mask


def intensity_moments(x, mask=None):
    """Per-volume moments on the device: a (B, 8) float64 tensor [count, non-finite count, min, max, mean, unbiased variance, 0, 0]
    over the voxels of each row of `x` (float32; a 1-D tensor is one volume, anything else a batch along its first axis) that `mask`
    (bool / uint8, same shape) counts.  min, max, mean and variance describe the finite counted voxels."""
    rows, mask = _intensity_rows("intensity_moments", x, mask)
    L = _lib.lib()
    b, n = rows.shape
    out = torch.empty((b, 8), dtype=torch.float64, device=rows.device)
    ws = _workspace(L.mri3d_intensity_workspace_bytes(n, b, 0), rows.device)
    check(L.mri3d_intensity_moments_f32(_ptr(rows), _ptr(mask), n, b, _ptr(out), _ptr(ws), ws.numel(), _stream()), "intensity_moments")
    return out


def _bandwidth_rule(bw_method):
    if bw_method is None or bw_method == "scott":
        return _lib.BW_SCOTT, 0.0
    if bw_method == "silverman":
        return _lib.BW_SILVERMAN, 0.0
    if isinstance(bw_method, str) or callable(bw_method):
        raise ValueError("gaussian_kde: bw_method must be None, 'scott', 'silverman' or a positive number, got %r" % (bw_method,))
    factor = float(bw_method)
    if not (factor > 0.0 and factor < float("inf")):
        raise ValueError("gaussian_kde: the bandwidth factor must be positive and finite, got %r" % (bw_method,))
    return _lib.BW_FACTOR, factor


def gaussian_kde(x, num_positions=100, positions=None, bw_method=None, mask=None, moments=None):
    """scipy.stats.gaussian_kde(values, bw_method)(positions) for every volume of a batch, on the device: (positions, density), two
    (B, m) float64 tensors.  `positions` None is np.linspace(min, max, num_positions) of each volume's counted voxels, bit for bit;
    else a 1-D float64 device tensor shared by all volumes.  `bw_method` None / 'scott' / 'silverman' / a number (the factor), as
    in scipy.  Where scipy has no answer (fewer than 2 counted voxels, no variance, a non-finite voxel) the densities are NaN.
    `moments` takes the result of `intensity_moments(x, mask)` when the caller already has it."""
    rows, mask = _intensity_rows("gaussian_kde", x, mask)
    rule, factor = _bandwidth_rule(bw_method)
    L = _lib.lib()
    b, n = rows.shape
    if positions is not None:
        if not positions.is_cuda or positions.dtype != torch.float64 or positions.dim() != 1:
            raise RuntimeError("gaussian_kde: positions must be a 1-D float64 ROCm device tensor (got %s %s on %s); there is no CPU "
                               "fallback" % (tuple(positions.shape), positions.dtype, positions.device))
        positions = positions.contiguous()
    m = int(num_positions) if positions is None else positions.numel()
    if moments is None:
        moments = intensity_moments(rows, mask)
    elif tuple(moments.shape) != (b, 8) or moments.dtype != torch.float64 or not moments.is_cuda or not moments.is_contiguous():
        raise RuntimeError("gaussian_kde: moments must be the contiguous (%d, 8) float64 device tensor of intensity_moments" % b)
    pos_out = torch.empty((b, max(m, 0)), dtype=torch.float64, device=rows.device)
    density = torch.empty((b, max(m, 0)), dtype=torch.float64, device=rows.device)
    ws = _workspace(L.mri3d_intensity_workspace_bytes(n, b, m), rows.device)
    check(L.mri3d_kde_f32(_ptr(rows), _ptr(mask), n, b, _ptr(moments), _ptr(positions), m, rule, factor, _ptr(pos_out), _ptr(density),
                          _ptr(ws), ws.numel(), _stream()), "kde")
    return pos_out, density


# ----------------------------------------------------------------------------------------------- registration (csrc/register.hip)
JOINT_HIST_PLAN_FIELDS = ("blocks", "groups", "group_candidates", "rows_per_trip", "trips", "lds_bytes", "stages", "wave_step")
HIST_COST_KINDS = {"corratio": 0, "mi": 1, "nmi": 2}
_RESAMPLE_LABEL_DTYPES = (torch.uint8, torch.int8, torch.bool, torch.int16, torch.int32)


def _volume(who, what, t, dtypes):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype not in dtypes:
        raise RuntimeError("%s: %s must be a %s ROCm device tensor (got %s on %s); there is no CPU fallback"
                           % (who, what, "/".join(str(d) for d in dtypes), getattr(t, "dtype", type(t)), getattr(t, "device", "host")))
    if t.dim() != 3 or t.numel() == 0:
        raise RuntimeError("%s: %s must be a non-empty (d, h, w) volume, got shape %s" % (who, what, tuple(t.shape)))
    return t.contiguous()


def _affines(who, affines, device):
    """(k, 3, 4) fixed-voxel -> moving-voxel matrices as a contiguous fp32 device tensor (host arrays and float64 are converted)."""
    a = torch.as_tensor(affines)
    if a.dim() == 2:
        a = a[None]
    if a.dim() != 3 or tuple(a.shape[1:]) != (3, 4) or a.shape[0] == 0:
        raise RuntimeError("%s: affines must be (k, 3, 4) or (3, 4), got shape %s" % (who, tuple(a.shape)))
    return a.to(device=device, dtype=torch.float32).contiguous()


def quantize_bins(x, lo, scale, bins, mask=None):
    """Histogram bin of every voxel of a float32 device tensor as uint8: clamp(floor((x - lo) * scale), 0, bins - 1), and 255
    ("skip") where `mask` (bool / uint8, same shape) is zero or x is not finite.  2 <= bins <= 64."""
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError("quantize_bins: needs a float32 ROCm device tensor (got %s on %s); there is no CPU fallback" % (x.dtype, x.device))
    x = x.contiguous()
    if mask is not None:
        if not mask.is_cuda or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != tuple(x.shape):
            raise RuntimeError("quantize_bins: the mask must be a bool / uint8 device tensor of shape %s (got %s %s on %s)"
                               % (tuple(x.shape), tuple(mask.shape), mask.dtype, mask.device))
        mask = mask.contiguous().view(torch.uint8)
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(_lib.lib().mri3d_quantize_u8(_ptr(x), _ptr(mask), x.numel(), float(lo), float(scale), int(bins), _ptr(out), _stream()),
          "quantize_u8")
    return out


def joint_hist_plan(fixed_shape, k, bins):
    """What one `joint_histogram` launch is built from, as a dict over JOINT_HIST_PLAN_FIELDS (host only)."""
    d, h, w = (int(s) for s in fixed_shape)
    out = (ctypes.c_int32 * 8)()
    check(_lib.lib().mri3d_joint_hist_plan(d, h, w, int(k), int(bins), out), "joint_hist_plan")
    return dict(zip(JOINT_HIST_PLAN_FIELDS, (int(v) for v in out)))


def joint_histogram(fixed_bins, moving, affines, m_lo, m_scale, bins, out=None):
    """Joint histograms of a quantised fixed volume (uint8 from `quantize_bins`, 255 = skip) and a float32 moving volume sampled
    trilinearly under each of k <= 64 candidate affines ((k, 3, 4), fixed voxel index -> moving voxel index): an int64 (k, bins, bins)
    device tensor, hist[c][fixed bin][moving bin].  Samples outside the moving volume are not counted."""
    fixed_bins = _volume("joint_histogram", "fixed_bins", fixed_bins, (torch.uint8,))
    moving = _volume("joint_histogram", "moving", moving, (torch.float32,))
    affines = _affines("joint_histogram", affines, moving.device)
    k, bins = affines.shape[0], int(bins)
    if out is None:
        out = torch.empty((k, max(bins, 0), max(bins, 0)), dtype=torch.int64, device=moving.device)
    elif tuple(out.shape) != (k, bins, bins) or out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous():
        raise RuntimeError("joint_histogram: out must be a contiguous (%d, %d, %d) int64 device tensor" % (k, bins, bins))
    L = _lib.lib()
    df, hf, wf = fixed_bins.shape
    dm, hm, wm = moving.shape
    ws = _workspace(L.mri3d_joint_hist_workspace_bytes(df, hf, wf, k, bins), moving.device)
    check(L.mri3d_joint_hist(_ptr(fixed_bins), df, hf, wf, _ptr(moving), dm, hm, wm, _ptr(affines), k, float(m_lo), float(m_scale), bins,
                             _ptr(out), _ptr(ws), ws.numel(), _stream()), "joint_hist")
    return out


def histogram_costs(hist, kind="corratio", min_count=0):
    """Similarity costs of (k, bins, bins) int64 joint histograms on the device: a (k, 2) float64 tensor of {cost, counted samples}.
    kind: 'corratio' (FLIRT's default), 'mi' (minus the mutual information) or 'nmi' (minus (H_f + H_m) / H_fm), or 0, 1, 2.
    The cost is +inf below `min_count` samples or where the measure's denominator vanishes."""
    if not hist.is_cuda or hist.dtype != torch.int64 or hist.dim() != 3 or hist.shape[1] != hist.shape[2] or hist.shape[0] == 0:
        raise RuntimeError("histogram_costs: needs a (k, bins, bins) int64 ROCm device tensor (got %s %s on %s); there is no CPU fallback"
                           % (tuple(hist.shape), hist.dtype, hist.device))
    if isinstance(kind, str):
        if kind not in HIST_COST_KINDS:
            raise ValueError("histogram_costs: kind must be one of %s, got %r" % (sorted(HIST_COST_KINDS), kind))
        kind = HIST_COST_KINDS[kind]
    hist = hist.contiguous()
    out = torch.empty((hist.shape[0], 2), dtype=torch.float64, device=hist.device)
    check(_lib.lib().mri3d_hist_costs(_ptr(hist), hist.shape[0], hist.shape[1], int(kind), float(min_count), _ptr(out), _stream()),
          "hist_costs")
    return out


def resample_affine(image=None, label=None, affine=None, out_shape=None, pad=0.0):
    """Resample a (d, h, w) float32 image (trilinear) and / or a label map (nearest; uint8, int8, bool, int16 or int32) onto a grid of
    `out_shape` under one (3, 4) affine from a destination voxel index to a source voxel index.  Outside the source the image gets
    `pad` and the label 0.  Returns (image_out, label_out), None where no input was given."""
    if image is None and label is None:
        raise RuntimeError("resample_affine: neither an image nor a label map given")
    if out_shape is None or len(tuple(out_shape)) != 3:
        raise RuntimeError("resample_affine: out_shape must be (d, h, w), got %r" % (out_shape,))
    df, hf, wf = (int(s) for s in out_shape)
    if image is not None:
        image = _volume("resample_affine", "image", image, (torch.float32,))
    if label is not None:
        label = _volume("resample_affine", "label", label, _RESAMPLE_LABEL_DTYPES)
        if image is not None and (tuple(label.shape) != tuple(image.shape) or label.device != image.device):
            raise RuntimeError("resample_affine: image %s and label %s differ in shape or device" % (tuple(image.shape), tuple(label.shape)))
    src = image if image is not None else label
    affine = _affines("resample_affine", affine, src.device)
    if affine.shape[0] != 1:
        raise RuntimeError("resample_affine: one (3, 4) affine expected, got %d" % affine.shape[0])
    dm, hm, wm = src.shape
    image_out = torch.empty((max(df, 0), max(hf, 0), max(wf, 0)), dtype=torch.float32, device=src.device) if image is not None else None
    label_out = torch.empty((max(df, 0), max(hf, 0), max(wf, 0)), dtype=label.dtype, device=src.device) if label is not None else None
    check(_lib.lib().mri3d_resample_affine(_ptr(image), _ptr(image_out), _ptr(label), _ptr(label_out),
                                           label.element_size() if label is not None else 0, dm, hm, wm, df, hf, wf, _ptr(affine),
                                           float(pad), _stream()), "resample_affine")
    return image_out, label_out


def downsample2(x):
    """One level of the image pyramid: a (ceil(d/2), ceil(h/2), ceil(w/2)) float32 volume, each voxel the mean of the 1-8 voxels of
    its 2x2x2 cell of `x` that exist."""
    x = _volume("downsample2", "x", x, (torch.float32,))
    d, h, w = x.shape
    y = torch.empty(((d + 1) // 2, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=x.device)
    check(_lib.lib().mri3d_downsample2_mean_f32(_ptr(x), d, h, w, _ptr(y), _stream()), "downsample2_mean")
    return y


# ----------------------------------------------------------------------------------------------- tissue classes (csrc/tissue.hip)
TISSUE_EM_PLAN_FIELDS = ("blocks", "rows_per_trip", "trips", "wave_steps", "row_sums", "entries", "fold_threads", "rows")


def tissue_coefficients(order):
    """Terms of a polynomial field of `order`: (order + 1)(order + 2)(order + 3) / 6."""
    return (order + 1) * (order + 2) * (order + 3) // 6


def tissue_table_size(classes, order):
    """Entries of the sums table of one EM pass: n, LL, S0/S1/S2 per class, the moments of w up to 2 * order and of t up to order."""
    return 2 + 3 * classes + tissue_coefficients(2 * order) + tissue_coefficients(order)


def _tissue_args(who, x, mask, classes, order, params):
    """The checked volume and mask (the caller holds them over its launch), and the eight arguments every C entry of the family starts
    with: x, mask, d, h, w, classes, order, params."""
    import numpy as np
    x = _volume(who, "x", x, (torch.float32,))
    if mask is not None:
        mask = _volume(who, "mask", mask, (torch.uint8, torch.bool))
        if tuple(mask.shape) != tuple(x.shape) or mask.device != x.device:
            raise RuntimeError("%s: x %s and mask %s differ in shape or device" % (who, tuple(x.shape), tuple(mask.shape)))
        mask = mask.view(torch.uint8)
    classes, order = int(classes), int(order)
    p = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
    if 2 <= classes <= 4 and 0 <= order <= 3 and p.size != 3 * classes + tissue_coefficients(order):
        raise ValueError("%s: %d classes and order %d take %d parameters (pi, mu, v, c), got %d"
                         % (who, classes, order, 3 * classes + tissue_coefficients(order), p.size))
    return x, mask, (_ptr(x), _ptr(mask), *x.shape, classes, order, p.ctypes.data_as(ctypes.c_void_p))     # the pointer keeps p alive


def tissue_em_plan(shape, classes, order):
    """What one `tissue_em_pass` launch is built from, as a dict over TISSUE_EM_PLAN_FIELDS (host only)."""
    d, h, w = (int(s) for s in shape)
    out = (ctypes.c_int32 * 8)()
    check(_lib.lib().mri3d_tissue_em_plan(d, h, w, int(classes), int(order), out), "tissue_em_plan")
    return dict(zip(TISSUE_EM_PLAN_FIELDS, (int(v) for v in out)))


def _tissue_pass_args(who, x, mask, classes, order, params, out):
    """What the two sums passes share: `_tissue_args`, then the sums tensor and the workspace."""
    x, mask, head = _tissue_args(who, x, mask, classes, order, params)
    d, h, w, classes, order = head[2:7]
    size = tissue_table_size(classes, order) if 2 <= classes <= 4 and 0 <= order <= 3 else 1
    out = _out_like(who, out, (size,), torch.float64, x)
    return x, mask, head, out, _workspace(_lib.lib().mri3d_tissue_em_workspace_bytes(d, h, w, classes, order), x.device)


def tissue_em_pass(x, mask, classes, order, params, out=None):
    """One EM pass of the tissue-class bias-field model over a float32 (d, h, w) device volume with the parameters fixed: the
    float64 device table (n, LL, S0[K], S1[K], S2[K], Mw, Mt) that include/mri3d.h documents.  mask: uint8 / bool device volume
    or None; params: 3K + M host doubles (pi, mu, v, c)."""
    x, mask, head, out, ws = _tissue_pass_args("tissue_em_pass", x, mask, classes, order, params, out)
    check(_lib.lib().mri3d_tissue_em_pass(*head, _ptr(out), _ptr(ws), ws.numel(), _stream()), "tissue_em_pass")
    return out


def tissue_mrf_pass(x, mask, classes, order, params, beta, mode, labels_in, labels_out=None, out=None):
    """`tissue_em_pass` with a Potts prior of strength `beta` on a uint8 label volume (0: not selected, else 1 + the class in the
    order of `params`), one half-sweep of red-black ICM: (sums, labels_out).  mode 0 / 1: the voxels of that colour of
    (d + h + w) & 1 take their new label, the others keep `labels_in`'s; mode 2, the start: no neighbour term, `labels_in` may be
    None.  `labels_out` is another buffer than `labels_in` (include/mri3d.h says why)."""
    x, mask, head, out, ws = _tissue_pass_args("tissue_mrf_pass", x, mask, classes, order, params, out)
    if labels_out is None:
        labels_out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    for name, t in (("labels_in", labels_in), ("labels_out", labels_out)):
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != tuple(x.shape) or t.dtype != torch.uint8 or t.device != x.device
                              or not t.is_contiguous()):
            raise RuntimeError("tissue_mrf_pass: %s must be a contiguous %s uint8 tensor on x's device" % (name, tuple(x.shape)))
    check(_lib.lib().mri3d_tissue_mrf_pass(*head, float(beta), int(mode), _ptr(labels_in), _ptr(labels_out), _ptr(out), _ptr(ws), ws.numel(),
                                           _stream()), "tissue_mrf_pass")
    return out, labels_out


def tissue_apply(x, mask, classes, order, params, want_field=False, restored=None):
    """The final pass: (restored = x exp(-b), labels uint8, field = exp(b) or None) over every voxel; labels are 0 where the voxel
    is not selected and else 1 + the rank by ascending mean of its most probable class.  `restored` may be `x` itself."""
    x, mask, head = _tissue_args("tissue_apply", x, mask, classes, order, params)
    if restored is None:
        restored = torch.empty_like(x)
    elif tuple(restored.shape) != tuple(x.shape) or restored.dtype != torch.float32 or not restored.is_cuda or not restored.is_contiguous():
        raise RuntimeError("tissue_apply: restored must be a contiguous %s float32 device tensor" % (tuple(x.shape),))
    labels = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    field = torch.empty_like(x) if want_field else None
    check(_lib.lib().mri3d_tissue_apply(*head, _ptr(restored), _ptr(labels), _ptr(field), _stream()), "tissue_apply")
    return restored, labels, field


# ----------------------------------------------------------------------------------------------- cat / add


class _CatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *xs):
        _require_device(*xs)
        L = _lib.lib()
        xs = [_cl(x) for x in xs]
        n, _, d, h, w = xs[0].shape
        es = xs[0].element_size()
        for x in xs:
            if x.dtype != xs[0].dtype:
                raise RuntimeError("cat_channels: dtypes differ: %s" % [t.dtype for t in xs])
            if (x.shape[0], x.shape[2], x.shape[3], x.shape[4]) != (n, d, h, w):
                raise RuntimeError("cat_channels: spatial/batch sizes differ: %s" % [tuple(t.shape) for t in xs])
        ctot = sum(x.shape[1] for x in xs)
        y = _new((n, ctot, d, h, w), xs[0])
        off = 0
        for x in xs:
            c = x.shape[1]
            check(L.mri3d_copy_channels(_ptr(x), _ptr(y, off * es), n * d * h * w, c, c, ctot, _dt(x), _stream()),
                  "copy_channels")
            off += c
        ctx.chans = [x.shape[1] for x in xs]
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        dy = _cl(dy)
        n, ctot, d, h, w = dy.shape
        outs = []
        off = 0
        for i, c in enumerate(ctx.chans):
            if ctx.needs_input_grad[i]:
                dx = _new((n, c, d, h, w), dy)
                check(L.mri3d_copy_channels(_ptr(dy, off * dy.element_size()), _ptr(dx), n * d * h * w, c, ctot, c, _dt(dy),
                                            _stream()), "copy_channels")
                outs.append(dx)
            else:
                outs.append(None)
            off += c
        return tuple(outs)


def cat_channels(xs):
    return _CatFn.apply(*xs)


def activation_dtype(x):
    """Storage type conv outputs (and everything downstream) will have for input x: bf16 inside `autocast()`."""
    return _autocast_dtype if _autocast_dtype is not None else x.dtype


def new_cat_buffer(n, channels, spatial, like):
    """Uninitialised NDHWC buffer that producers fill slice by slice (norm_act(out=), upsample3d(out=))."""
    return torch.empty((n, channels, *spatial), dtype=activation_dtype(like), device=like.device, memory_format=CL3D)


class _JoinFn(torch.autograd.Function):
    """torch.cat(dim=1) WITHOUT the copy: the parts are channel-slice views that their producers already wrote into
    `buf`; forward hands out the buffer, backward hands each producer its slice of the gradient (views, no copy)."""

    @staticmethod
    def forward(ctx, buf, *parts):
        off = 0
        for p in parts:
            c = p.shape[1]
            if p.data_ptr() != buf.data_ptr() + off * buf.element_size() or _pitch_of(p) != buf.shape[1]:
                raise RuntimeError("join_channels: part is not the [%d:%d) channel slice of the buffer" % (off, off + c))
            off += c
        if off != buf.shape[1]:
            raise RuntimeError("join_channels: parts cover %d of %d channels" % (off, buf.shape[1]))
        ctx.chans = [p.shape[1] for p in parts]
        return buf.view_as(buf)

    @staticmethod
    def backward(ctx, dcat):
        dcat, _ = _nd(dcat)
        if _pitch_of(dcat) != dcat.shape[1]:
            dcat = dcat.contiguous(memory_format=CL3D)
        outs, off = [None], 0
        for c in ctx.chans:
            outs.append(_slice_view(dcat, off, c))
            off += c
        return tuple(outs)


def join_channels(buf, parts):
    return _JoinFn.apply(buf, *parts)


class _AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _require_device(a, b)
        L = _lib.lib()
        a = _cl(a)
        b = _cl(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            raise RuntimeError("add: shapes/dtypes differ %s %s vs %s %s" % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype))
        n, c, d, h, w = a.shape
        y = _new(a.shape, a)
        check(L.mri3d_add_channels(_ptr(a), _ptr(b), _ptr(y), n * d * h * w, c, c, c, c, _dt(a), _stream()), "add_channels")
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add(a, b):
    return _AddFn.apply(a, b)
