"""MI355X-native drop-in for the three blocks of segmentation/models/3d_bayes_layers.py that its U-Net is built from
(ConvBlock :16-35, BasicDownBlock :38-57, BasicUpBlock :60-76): same constructor arguments, same attribute names and so the
same state_dict keys (`conv.2.*`, `conv_1`, `conv_2`, `down`, `upsample.0`).  The reference's file name starts with a digit and
cannot be imported as a module; this one is `bayes_layers`.

InstanceNorm3d -> ReLU runs as one fused HIP pass, the convolution is `nn.Conv3d` or `nn.BayesConv3d` (bayes=True), residual
sums are `ops.add`, the x2 trilinear upsampling (align_corners=True) is `nn.Upsample`.  BayesConv2d, ConvSample, Conv_Layer,
Up_Conv and the other classes of the reference file are not used by the U-Net and are not provided.
"""
import torch.nn as tnn

from ... import nn as mnn
from ... import ops
from ...nn import BayesConv3d  # noqa: F401  (the reference's layers module defines it; `from .bayes_layers import *` users find it)


class ConvBlock(tnn.Module):
    """InstanceNorm3d => ReLU => conv (pre-activation)."""

    def __init__(self, in_channels, out_channels, kernel, stride, padding=1, bayes=False):
        super().__init__()
        conv = mnn.BayesConv3d if bayes else mnn.Conv3d
        self.conv = tnn.Sequential(
            mnn.InstanceNorm3d(in_channels),
            mnn.ReLU(inplace=True),
            conv(in_channels, out_channels, kernel_size=kernel, stride=stride, padding=padding, bias=False))

    def forward(self, x):
        return self.conv[2](mnn.fused_norm_act(self.conv[0], self.conv[1], x))


class BasicDownBlock(tnn.Module):
    def __init__(self, in_channels, out_channels, downsample, bayes=False):
        super().__init__()
        self.conv_1 = ConvBlock(in_channels, out_channels, kernel=3, stride=2 if downsample else 1, bayes=bayes)
        self.conv_2 = ConvBlock(out_channels, out_channels, kernel=3, stride=1, bayes=bayes)
        self.down = ConvBlock(in_channels, out_channels, kernel=1, stride=2, padding=0, bayes=False) if downsample else None

    def forward(self, inp):
        x = self.conv_2(self.conv_1(inp))
        return ops.add(x, self.down(inp) if self.down is not None else inp)


class BasicUpBlock(tnn.Module):
    def __init__(self, in_channels, out_channels, upsample=True, bayes=False):
        super().__init__()
        self.upsample = tnn.Sequential(ConvBlock(in_channels, out_channels, kernel=1, stride=1, padding=0, bayes=False),
                                       mnn.Upsample(scale_factor=2, mode="trilinear", align_corners=True))
        self.conv_1 = ConvBlock(out_channels, out_channels, kernel=3, stride=1, bayes=bayes)
        self.conv_2 = ConvBlock(out_channels, out_channels, kernel=3, stride=1, bayes=bayes)

    def forward(self, inp, skip_connection=None):
        x = self.upsample(inp)
        if skip_connection is not None:
            x = ops.add(x, skip_connection)
        return ops.add(self.conv_2(self.conv_1(x)), x)
