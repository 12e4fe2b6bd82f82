"""Drop-in ``torch.nn`` layer classes whose forward/backward run on the HIP kernels.

Each class subclasses its ``torch.nn`` namesake, so constructor signatures, parameter initialisation and
``state_dict`` keys are identical to what the reference models create; only ``forward`` is replaced.
``fused_norm_act`` applies a normalisation layer and the activation that follows it in ONE kernel pass — the
conv -> BatchNorm3d -> PReLU blocks of ``unet.UNet`` and the (MaxPool ->) BatchNorm3d -> LeakyReLU tails of
``AE_model.DownBlock`` (classification/models/AE_model.py:27-36) — and ``FusedSequential`` does that pairing
automatically for ``nn.Sequential``-style reference models (classification/models/cnn_model.py:104-175).
"""
import math

import torch
import torch.nn as tnn

from . import ops


class Conv3d(tnn.Conv3d):
    def forward(self, x):
        if self.padding_mode != "zeros" or self.groups != 1 or isinstance(self.padding, str):
            raise NotImplementedError("mri3d Conv3d supports padding_mode='zeros', groups=1, numeric padding")
        return ops.conv3d(x, self.weight, self.bias, self.stride, self.padding, self.dilation)


class ConvTranspose3d(tnn.ConvTranspose3d):
    def forward(self, x, output_size=None):
        if output_size is not None or self.groups != 1 or self.padding_mode != "zeros":
            raise NotImplementedError("mri3d ConvTranspose3d supports groups=1, zero padding, no output_size")
        return ops.conv_transpose3d(x, self.weight, self.bias, self.stride, self.padding, self.output_padding,
                                    self.dilation)


class BayesConv3d(tnn.Module):
    """Variational-dropout convolution (segmentation/models/3d_bayes_layers.py:85-116,195-232): same constructor, parameters
    (`mu_weight`, `logsigma_weight`, `mu_bias`, `logsigma_bias`), initialisation and state_dict keys; `forward` is
    `ops.bayes_conv3d` and leaves `self.log_alpha` behind for a KL regulariser, as the reference does.

    `noise`: None (the operator draws the standard normals from torch's device generator) or a callable
    `(shape, device) -> eps`, eps a float32 tensor of the output's (N, Co, D, H, W) shape — how a test, or a caller that wants
    the same sample twice, supplies the noise.  A plain attribute, not part of the state_dict."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 zero_mean=False, threshold=3):
        super().__init__()
        if in_channels % groups != 0 or out_channels % groups != 0:
            raise ValueError("in_channels and out_channels must be divisible by groups")
        self.in_channels, self.out_channels, self.groups = in_channels, out_channels, groups
        self.kernel_size, self.stride, self.dilation = ops._triple(kernel_size), ops._triple(stride), ops._triple(dilation)
        self.padding = padding if isinstance(padding, str) else ops._triple(padding)
        self.zero_mean, self.threshold = zero_mean, threshold
        self.noise = None
        self.log_alpha = None
        shape = (out_channels, in_channels // groups) + self.kernel_size
        self.mu_weight = tnn.Parameter(torch.empty(shape))
        self.logsigma_weight = tnn.Parameter(torch.empty(shape))
        if bias:
            self.mu_bias = tnn.Parameter(torch.empty(out_channels))
            self.logsigma_bias = tnn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("mu_bias", None)
            self.register_parameter("logsigma_bias", None)
        self.reset_parameters()
        if zero_mean:
            self.mu_weight = tnn.Parameter(torch.zeros_like(self.mu_weight))

    def reset_parameters(self):
        with torch.no_grad():
            self.mu_weight.normal_(0, 0.02)
            self.logsigma_weight.fill_(-5)
            if self.mu_bias is not None:
                fan_in = self.mu_weight[0].numel()
                bound = 1 / math.sqrt(fan_in)
                self.mu_bias.uniform_(-bound, bound)
                self.logsigma_bias.uniform_(-bound, bound)

    def output_shape(self, x):
        """(N, Co, D, H, W) of forward(x): what `noise` is asked for."""
        return (x.shape[0], self.out_channels) + tuple(
            (i + 2 * p - d * (k - 1) - 1) // s + 1
            for i, p, d, k, s in zip(x.shape[2:], self.padding, self.dilation, self.kernel_size, self.stride))

    def extra_repr(self):
        return "%d, %d, kernel_size=%s, stride=%s, padding=%s%s" % (self.in_channels, self.out_channels, self.kernel_size, self.stride,
                                                                    self.padding, "" if self.mu_bias is not None else ", bias=False")

    def forward(self, x):
        if self.groups != 1 or isinstance(self.padding, str):
            raise NotImplementedError("mri3d BayesConv3d supports groups=1, numeric padding")
        eps = self.noise(self.output_shape(x), x.device) if self.noise is not None else None
        y, self.log_alpha = ops.bayes_conv3d(x, self.mu_weight, self.logsigma_weight, self.mu_bias, self.logsigma_bias, self.stride,
                                             self.padding, self.dilation, self.training, self.threshold, eps)
        return y


def _act_spec(act):
    """(kind, alpha tensor or None, slope) for an activation module (or None)."""
    if act is None or isinstance(act, tnn.Identity):
        return None, None, 0.0
    if isinstance(act, tnn.PReLU):
        return "prelu", act.weight, 0.0
    if isinstance(act, tnn.LeakyReLU):
        return "leaky_relu", None, float(act.negative_slope)
    if isinstance(act, tnn.ReLU):
        return "relu", None, 0.0
    raise NotImplementedError("unsupported activation module %r" % (act,))


def _batchnorm_spec(norm, alpha):
    """(mode, leading arguments of ops.norm_act and the fused operators) for a BatchNorm3d: "batch" or "running" statistics, or
    "sync" where a training layer takes them over all ranks."""
    use_batch = norm.training or norm.running_mean is None
    mode = "running" if not use_batch else ("sync" if norm.training and ops.sync_batchnorm_reducer() is not None else "batch")
    running = (norm.running_mean, norm.running_var) if norm.track_running_stats else (None, None)
    return mode, (norm.weight, norm.bias, alpha, *running, mode, norm.momentum, norm.eps)


def _count_batch(norm):
    if norm is not None and norm.training and norm.track_running_stats and norm.num_batches_tracked is not None:
        norm.num_batches_tracked.add_(1)


def fused_norm_act(norm, act, x, out=None):
    """act(norm(x)) in one pass.  `norm` is a BatchNorm3d / InstanceNorm3d module or None; `act` an activation or None.
    `out=(buffer, channel_offset)` makes the kernel write straight into a channel slice of a wider NDHWC buffer (a
    decoder concat buffer) and returns that slice as a view."""
    kind, alpha, slope = _act_spec(act)
    if norm is None:
        if kind is None and out is None:
            return x
        return ops.norm_act(x, None, None, alpha, None, None, "none", 0.1, 0.0, kind, slope, out)
    if isinstance(norm, tnn.modules.batchnorm._BatchNorm):
        _count_batch(norm)
        return ops.norm_act(x, *_batchnorm_spec(norm, alpha)[1], kind, slope, out)
    if isinstance(norm, tnn.modules.instancenorm._InstanceNorm):
        if norm.track_running_stats:
            raise NotImplementedError("InstanceNorm3d(track_running_stats=True) is not supported")
        return ops.norm_act(x, norm.weight, norm.bias, alpha, None, None, "instance", 0.1, norm.eps, kind, slope, out)
    if isinstance(norm, tnn.GroupNorm):
        return ops.norm_act(x, norm.weight, norm.bias, alpha, None, None, "group", 0.1, norm.eps, kind, slope, out,
                            norm.num_channels // norm.num_groups)
    raise NotImplementedError("unsupported normalisation module %r" % (norm,))


def _plain_pointwise(head):
    return (isinstance(head, Conv3d) and tuple(head.kernel_size) == (1, 1, 1) and tuple(head.stride) == (1, 1, 1)
            and tuple(head.dilation) == (1, 1, 1) and head.groups == 1 and head.padding_mode == "zeros"
            and not isinstance(head.padding, str) and tuple(head.padding) == (0, 0, 0))


def _local_stats_spec(norm, act):
    """(mode, leading arguments of the fused operators, activation kind, alpha, slope) for `norm` a BatchNorm3d with local batch or
    running statistics, or None (activation only); None for every other normalisation (instance, group, synchronised)."""
    kind, alpha, slope = _act_spec(act)
    if norm is None:
        return "none", (None, None, alpha, None, None, "none", 0.1, 0.0), kind, alpha, slope
    if not isinstance(norm, tnn.modules.batchnorm._BatchNorm) or norm.momentum is None:
        return None
    mode, args = _batchnorm_spec(norm, alpha)
    return None if mode == "sync" else (mode, args, kind, alpha, slope)


def _fused_tail(norm, act, supported, asked, run, given):
    """The shared end of the two folds below: run(*given, ...) where supported(*asked, ...) serves the layer, after counting the
    batch as the layer's own forward would; None, with nothing touched, where it does not."""
    spec = _local_stats_spec(norm, act)
    if spec is None:
        return None
    mode, args, kind, alpha, slope = spec
    if not supported(*asked, mode, kind, alpha):
        return None
    _count_batch(norm)
    return run(*given, *args, act=kind, slope=slope)


def fused_norm_act_head(norm, act, x, head):
    """head(act(norm(x))) as ONE operator (ops.norm_act_pointwise) where that is served: `head` a plain 1x1x1 Conv3d with at most
    four output channels, `norm` a BatchNorm3d with local batch or running statistics (or None), channels and layout as the native
    predicate asks.  Returns None — with nothing run and no counter touched — where it is not: the caller keeps the two operators."""
    if not _plain_pointwise(head):
        return None
    cast = ops.autocast_dtype()
    if cast is not None and x.dtype != cast:   # the head's conv3d would convert its input first
        return None
    return _fused_tail(norm, act, ops.norm_act_pointwise_supported, (x, head.weight), ops.norm_act_pointwise,
                       (x, head.weight, head.bias))


def fused_norm_act_pool(norm, act, x, pool):
    """(pool(a), a) with a = act(norm(x)) as ONE operator (ops.norm_act_pool) where that is served: `pool` a MaxPool3d(2) in floor
    mode, `norm` a BatchNorm3d with local batch or running statistics (or None), fp32 activations, extents, channels and layout as
    the native predicate asks.  Returns None — with nothing run and no counter touched — where it is not: the caller keeps the two operators."""
    if (not isinstance(pool, tnn.MaxPool3d) or pool.ceil_mode or pool.return_indices or pool.dilation not in (1, (1, 1, 1))
            or not x.is_cuda):
        return None
    if x.dtype != torch.float32:
        # bf16 activations keep the two operators: measured on the bench step the fold is no faster there (DESIGN §4.6 — the
        # backward sums pass is bound by its float64 accumulation, not by the bytes the fold removes); ops.norm_act_pool serves bf16
        return None
    return _fused_tail(norm, act, ops.norm_act_pool_supported, (x, pool.kernel_size, pool.stride, pool.padding), ops.norm_act_pool,
                       (x,))


def fused_conv_act(conv, act, x):
    """act(conv(x)) as ONE operator (ops.conv3d_act) where that is served: `conv` a plain 3x3x3 Conv3d of one input channel with
    stride 1, padding 1 and dilation 1, `act` a PReLU, LeakyReLU or ReLU, x an fp32 device tensor nobody wants a gradient of, and the
    native predicate's yes.  Returns None — with nothing run — where it is not: the caller keeps the two operators."""
    if not (isinstance(conv, Conv3d) and conv.padding_mode == "zeros" and conv.groups == 1 and not isinstance(conv.padding, str)
            and tuple(conv.kernel_size) == (3, 3, 3) and tuple(conv.stride) == (1, 1, 1) and tuple(conv.padding) == (1, 1, 1)
            and tuple(conv.dilation) == (1, 1, 1) and torch.is_tensor(x)):
        return None
    kind, alpha, slope = _act_spec(act)
    if kind is None or not ops.conv3d_act_supported(x, conv.weight, kind, alpha):
        return None
    return ops.conv3d_act(x, conv.weight, conv.bias, alpha, kind, slope)


def conv_norm_act(conv, norm, act, x, out=None, head=None, pool=None, fused_first=True):
    """act(norm(conv(x))) for a Conv3d module followed by a normalisation (`unet.UNet`'s ConvolutionalBlock, the conv -> BN ->
    ReLU stems of cnn_model.py).  When `norm` is a BatchNorm3d that will use BATCH statistics (training mode, local statistics)
    the convolution is asked to accumulate them in its epilogue, which saves the statistics pass over its output.
    head: a Conv3d module applied to the result (`unet.UNet`'s 1x1x1 classifier); the return value is then head(act(norm(conv(x)))),
    computed without storing the activation where `fused_norm_act_head` serves the case.
    pool: a MaxPool3d module applied to the result, which is also kept (`unet.UNet`'s encoder levels); the return value is then
    (pool(a), a) for a = act(norm(conv(x))), from one operator where `fused_norm_act_pool` serves the case.
    fused_first: without a normalisation, out, head or pool, the convolution and its activation run as one operator where
    `fused_conv_act` serves the case (`unet.UNet`'s first layer)."""
    if fused_first and norm is None and out is None and head is None and pool is None:
        a = fused_conv_act(conv, act, x)
        if a is not None:
            return a
    wants =(isinstance(norm, tnn.modules.batchnorm._BatchNorm) and (norm.training or norm.running_mean is None)
             and ops.sync_batchnorm_reducer() is None and isinstance(conv, Conv3d) and conv.padding_mode == "zeros"
             and conv.groups == 1 and not isinstance(conv.padding, str))
    if isinstance(x, (tuple, list)):
        # x = (xa, xb): the convolution of torch.cat((xa, xb), dim=1), read from the two tensors (ops.conv3d_cat)
        xa, xb = x
        plain = (isinstance(conv, Conv3d) and conv.padding_mode == "zeros" and conv.groups == 1 and not isinstance(conv.padding, str)
                 and tuple(conv.stride) == (1, 1, 1) and tuple(conv.dilation) == (1, 1, 1))
        if plain:
            y = ops.conv3d_cat(xa, xb, conv.weight, conv.bias, conv.padding, bn_stats=wants)
        else:
            y = conv(ops.cat_channels([xa, xb]))
    elif wants:
        y = ops.conv3d(x, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, bn_stats=True)
    else:
        y = conv(x)
    if head is not None:
        logits = fused_norm_act_head(norm, act, y, head) if out is None else None
        return logits if logits is not None else head(fused_norm_act(norm, act, y, out))
    if pool is not None:
        both = fused_norm_act_pool(norm, act, y, pool) if out is None else None
        return both if both is not None else pool.forward_with_skip(fused_norm_act(norm, act, y, out))
    return fused_norm_act(norm, act, y, out)


class GroupNorm(tnn.GroupNorm):
    def forward(self, x):
        return fused_norm_act(self, None, x)


class BatchNorm3d(tnn.BatchNorm3d):
    def forward(self, x):
        return fused_norm_act(self, None, x)


class InstanceNorm3d(tnn.InstanceNorm3d):
    def forward(self, x):
        return fused_norm_act(self, None, x)


class PReLU(tnn.PReLU):
    def forward(self, x):
        if x.dim() != 5:  # classifier-head vectors (N, F): not on the volumetric path
            return super().forward(x)
        return fused_norm_act(None, self, x)


class ReLU(tnn.ReLU):
    def forward(self, x):
        if x.dim() != 5:  # classifier-head vectors (N, F): not on the volumetric path
            return super().forward(x)
        return fused_norm_act(None, self, x)


class LeakyReLU(tnn.LeakyReLU):
    def forward(self, x):
        if x.dim() != 5:  # classifier-head vectors (N, F): not on the volumetric path
            return super().forward(x)
        return fused_norm_act(None, self, x)


class MaxPool3d(tnn.MaxPool3d):
    def forward(self, x):
        if self.ceil_mode or self.return_indices or self.dilation not in (1, (1, 1, 1)):
            raise NotImplementedError("mri3d MaxPool3d supports floor mode, dilation 1, no indices")
        return ops.max_pool3d(x, self.kernel_size, self.stride, self.padding)

    def forward_with_skip(self, x):
        """(pool(x), x) as one autograd node — for blocks whose output also feeds a skip connection (ops.max_pool3d_skip)."""
        if self.ceil_mode or self.return_indices or self.dilation not in (1, (1, 1, 1)):
            raise NotImplementedError("mri3d MaxPool3d supports floor mode, dilation 1, no indices")
        return ops.max_pool3d_skip(x, self.kernel_size, self.stride, self.padding)


# 2-D layers (detection/model_utils.py:19-52): a (N, C, H, W) image is the (N, C, 1, H, W) volume of one slice, so the 3-D operators
# serve it as they are.  Each layer takes the 4-D tensor of its torch namesake and returns one, or takes the 5-D form with D = 1 and
# returns that: a model that stays in the 5-D form between its layers (detection.model.PatchModel) moves no data between layouts.
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _as_slice(x, who):
    """(x as (N, C, 1, H, W), whether it came as (N, C, H, W))."""
    if x.dim() == 4:
        return x.unsqueeze(2), True
    if x.dim() == 5 and x.shape[2] == 1:
        return x, False
    raise RuntimeError("mri3d %s expects (N, C, H, W) or (N, C, 1, H, W), got shape %s" % (who, tuple(x.shape)))


class Conv2d(tnn.Conv2d):
    def forward(self, x):
        if self.padding_mode != "zeros" or self.groups != 1 or isinstance(self.padding, str):
            raise NotImplementedError("mri3d Conv2d supports padding_mode='zeros', groups=1, numeric padding")
        x, four = _as_slice(x, "Conv2d")
        # the 4-D parameter stays the leaf (and the state_dict entry); its 5-D view is no GradSink owner, so the weight gradient goes
        # back through autograd into the parameter
        y = ops.conv3d(x, self.weight.unsqueeze(2), self.bias, (1,) + _pair(self.stride), (0,) + _pair(self.padding),
                       (1,) + _pair(self.dilation))
        return y.squeeze(2) if four else y


class BatchNorm2d(tnn.BatchNorm2d):
    def forward(self, x):
        x, four = _as_slice(x, "BatchNorm2d")
        y = fused_norm_act(self, None, x)
        return y.squeeze(2) if four else y


class MaxPool2d(tnn.MaxPool2d):
    def forward(self, x):
        if self.ceil_mode or self.return_indices or self.dilation not in (1, (1, 1)):
            raise NotImplementedError("mri3d MaxPool2d supports floor mode, dilation 1, no indices")
        x, four = _as_slice(x, "MaxPool2d")
        stride = self.kernel_size if self.stride is None else self.stride
        y = ops.max_pool3d(x, (1,) + _pair(self.kernel_size), (1,) + _pair(stride), (0,) + _pair(self.padding))
        return y.squeeze(2) if four else y


class Upsample(tnn.Upsample):
    def forward(self, x):
        return ops.upsample3d(x, self.size, self.scale_factor, self.mode, self.align_corners)


class Dropout3d(tnn.Dropout3d):
    def forward(self, x):
        return ops.dropout3d(x, self.p, self.training)


class Flatten(tnn.Module):
    """(N, C, D, H, W) -> (N, C*D*H*W) in torch's NCDHW element order (tiny tensors; a layout copy only)."""

    def forward(self, x):
        return x.contiguous(memory_format=torch.contiguous_format).view(x.size(0), -1)


_NORMS = (tnn.modules.batchnorm._BatchNorm, tnn.modules.instancenorm._InstanceNorm)
_ACTS = (tnn.PReLU, tnn.ReLU, tnn.LeakyReLU)


def run_fused(modules, x):
    """Run a list of modules like nn.Sequential, fusing 5-D [norm ->] activation pairs into one kernel."""
    mods = list(modules)
    i = 0
    while i < len(mods):
        m = mods[i]
        five_d = torch.is_tensor(x) and x.dim() == 5
        if (five_d and i == 0 and isinstance(m, Conv3d) and len(mods) > 2 and isinstance(mods[1], Conv3d) and isinstance(mods[2], Conv3d)
                and ops.conv3d_pair_supported(x, m, mods[1])):
            # the head of the autoencoder's first DownBlock on the network input: the gradient of the (k,1,1) convolution's output is
            # never formed (ops.conv3d_pair)
            x = ops.conv3d_pair(x, m, mods[1])
            i += 2
            continue
        if five_d and isinstance(m, Conv3d) and i + 1 < len(mods) and isinstance(mods[i + 1], tnn.BatchNorm3d):
            nxt2 = mods[i + 2] if i + 2 < len(mods) else None
            if isinstance(nxt2, _ACTS):
                x = conv_norm_act(m, mods[i + 1], nxt2, x)
                i += 3
            else:
                x = conv_norm_act(m, mods[i + 1], None, x)
                i += 2
            continue
        if five_d and isinstance(m, (tnn.BatchNorm3d, tnn.InstanceNorm3d, tnn.GroupNorm)):
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            if isinstance(nxt, _ACTS):
                x = fused_norm_act(m, nxt, x)
                i += 2
                continue
            x = fused_norm_act(m, None, x)
        elif five_d and isinstance(m, _ACTS):
            x = fused_norm_act(None, m, x)
        else:
            x = m(x)
        i += 1
    return x


class FusedSequential(tnn.Sequential):
    def forward(self, x):
        return run_fused(self, x)
