"""Pure-PyTorch restatement of the variational-dropout U-Net (reference segmentation/models/3d_bayes_layers.py::BayesConv3d,
ConvBlock, BasicDownBlock, BasicUpBlock and 3d_bayes_unet.py::UNet3D), written in this project's own words: the CPU yardstick
of tests/test_bayes_ref.py and tests/test_bayes_gpu.py.  tools/gen_bayes_golden.py asserts that it equals the reference bit for
bit when both are fed the same noise.  Works in float32 and float64.

Every BayesConv3d has the product's `noise` hook: None (draw standard normals) or a callable (shape, device) -> eps.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

LOG_EPS = 1e-8     # log(mu^2 + LOG_EPS)
VAR_EPS = 1e-4     # sqrt(VAR_EPS + var_out)


def weight_transform(mu, logsigma, training, threshold):
    """(w_mean, w_var, log_alpha) of the layer: the formula of the issue, differentiable by autograd."""
    log_alpha = torch.clamp(logsigma - torch.log(mu ** 2 + LOG_EPS), -5, 5)
    w_var = mu ** 2 * torch.exp(log_alpha)
    if training:
        return mu, w_var, log_alpha
    keep = (log_alpha < threshold).to(mu.dtype)
    return mu * keep, w_var * keep, log_alpha


def bayes_conv3d(x, mu, logsigma, mu_bias, logsigma_bias, stride, padding, dilation, training, threshold, eps):
    w_mean, w_var, log_alpha = weight_transform(mu, logsigma, training, threshold)
    var_bias = None if logsigma_bias is None else logsigma_bias.pow(2)
    std = torch.sqrt(VAR_EPS + F.conv3d(x.pow(2), w_var, var_bias, stride, padding, dilation))
    mean = F.conv3d(x, w_mean, mu_bias, stride, padding, dilation)
    return eps * std + mean, log_alpha


class BayesConv3d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, zero_mean=False,
                 threshold=3):
        super().__init__()
        assert groups == 1
        three = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3   # noqa: E731
        self.kernel_size, self.stride, self.padding, self.dilation = three(kernel_size), three(stride), three(padding), three(dilation)
        self.out_channels, self.threshold, self.noise, self.log_alpha = out_channels, threshold, None, None
        shape = (out_channels, in_channels) + self.kernel_size
        self.mu_weight = nn.Parameter(torch.empty(shape).normal_(0, 0.02))
        self.logsigma_weight = nn.Parameter(torch.full(shape, -5.0))
        if bias:
            bound = 1 / math.sqrt(in_channels * self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2])
            self.mu_bias = nn.Parameter(torch.empty(out_channels).uniform_(-bound, bound))
            self.logsigma_bias = nn.Parameter(torch.empty(out_channels).uniform_(-bound, bound))
        else:
            self.register_parameter("mu_bias", None)
            self.register_parameter("logsigma_bias", None)
        if zero_mean:
            self.mu_weight = nn.Parameter(torch.zeros(shape))

    def forward(self, x):
        out = tuple((i + 2 * p - d * (k - 1) - 1) // s + 1
                    for i, p, d, k, s in zip(x.shape[2:], self.padding, self.dilation, self.kernel_size, self.stride))
        shape = (x.shape[0], self.out_channels) + out
        eps = self.noise(shape, x.device) if self.noise is not None else torch.empty(shape, device=x.device).normal_()
        y, self.log_alpha = bayes_conv3d(x, self.mu_weight, self.logsigma_weight, self.mu_bias, self.logsigma_bias, self.stride,
                                         self.padding, self.dilation, self.training, self.threshold, eps.to(x.dtype))
        return y


def _conv(bayes, cin, cout, k, stride, pad):
    cls = BayesConv3d if bayes else nn.Conv3d
    return cls(cin, cout, kernel_size=k, stride=stride, padding=pad, bias=False)


class ConvBlock(nn.Module):
    def __init__(self, in_channels, out_channels, kernel, stride, padding=1, bayes=False):
        super().__init__()
        self.conv = nn.Sequential(nn.InstanceNorm3d(in_channels), nn.ReLU(), _conv(bayes, in_channels, out_channels, kernel, stride, padding))

    def forward(self, x):
        return self.conv(x)


class BasicDownBlock(nn.Module):
    def __init__(self, in_channels, out_channels, downsample, bayes=False):
        super().__init__()
        self.conv_1 = ConvBlock(in_channels, out_channels, 3, 2 if downsample else 1, bayes=bayes)
        self.conv_2 = ConvBlock(out_channels, out_channels, 3, 1, bayes=bayes)
        self.down = ConvBlock(in_channels, out_channels, 1, 2, padding=0) if downsample else None

    def forward(self, x):
        y = self.conv_2(self.conv_1(x))
        return y + (x if self.down is None else self.down(x))


class BasicUpBlock(nn.Module):
    def __init__(self, in_channels, out_channels, bayes=False):
        super().__init__()
        self.upsample = nn.Sequential(ConvBlock(in_channels, out_channels, 1, 1, padding=0),
                                      nn.Upsample(scale_factor=2, mode="trilinear", align_corners=True))
        self.conv_1 = ConvBlock(out_channels, out_channels, 3, 1, bayes=bayes)
        self.conv_2 = ConvBlock(out_channels, out_channels, 3, 1, bayes=bayes)

    def forward(self, x, skip=None):
        x = self.upsample(x)
        if skip is not None:
            x = x + skip
        return self.conv_2(self.conv_1(x)) + x


class UNet3D(nn.Module):
    def __init__(self, n_classes, n_channels=(1, 16, 32, 64, 128), bayes=False, shorten=False):
        super().__init__()
        c = list(n_channels)
        self.init_conv = _conv(bayes, c[0], c[1], 3, 1, 1)
        widths = [(c[1], c[2], True), (c[2], c[2], False), (c[2], c[3], True), (c[3], c[3], False), (c[3], c[4], True), (c[4], c[4], False)]
        widths += [] if shorten else [(c[4], c[4], False)] * 3
        for i, (cin, cout, down) in enumerate(widths, 1):
            setattr(self, "down%d" % i, BasicDownBlock(cin, cout, down, bayes=bayes))
        self.depth = len(widths)
        self.up1, self.up2, self.up3 = (BasicUpBlock(c[4], c[3], bayes=bayes), BasicUpBlock(c[3], c[2], bayes=bayes),
                                        BasicUpBlock(c[2], c[1], bayes=bayes))
        self.out = nn.Conv3d(c[1], n_classes, kernel_size=1, bias=False)

    def forward(self, x):
        x1 = self.init_conv(x)
        x2 = self.down2(self.down1(x1))
        x3 = self.down4(self.down3(x2))
        x4 = self.down5(x3)
        for i in range(6, self.depth + 1):
            x4 = getattr(self, "down%d" % i)(x4)
        return self.out(self.up3(self.up2(self.up1(x4, x3), x2), x1))


# ----------------------------------------------------------------------------------------------- noise plumbing for the tests
def bayes_layers(model):
    """The BayesConv3d-like modules of `model` (anything with a `noise` attribute and a `mu_weight`), in registration order."""
    return [m for m in model.modules() if hasattr(m, "noise") and hasattr(m, "mu_weight")]


class NoiseTape:
    """Feeds a fixed list of noise tensors, one per BayesConv3d call in call order, into every layer of a model; with no list,
    draws them from a seeded CPU generator and records them.  `install(model)` sets each layer's `noise` hook."""

    def __init__(self, tensors=None, seed=0):
        self.tensors = None if tensors is None else [torch.as_tensor(t) for t in tensors]
        self.recorded, self.pos = [], 0
        self.gen = torch.Generator().manual_seed(seed) if tensors is None else None

    def rewind(self):
        self.pos = 0
        return self

    def __call__(self, shape, device):
        if self.tensors is None and self.pos == len(self.recorded):
            self.recorded.append(torch.randn(*shape, generator=self.gen))
        src = self.tensors if self.tensors is not None else self.recorded
        eps = src[self.pos]
        assert tuple(eps.shape) == tuple(shape), (self.pos, tuple(eps.shape), tuple(shape))
        self.pos += 1
        return eps.to(device)

    def install(self, model):
        for layer in bayes_layers(model):
            layer.noise = self
        return self.rewind()
