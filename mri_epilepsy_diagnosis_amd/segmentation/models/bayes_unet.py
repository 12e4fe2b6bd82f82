"""MI355X-native drop-in for segmentation/models/3d_bayes_unet.py::UNet3D(n_classes, n_channels, bayes, devices, shorten): a
pre-activation residual 3-D U-Net whose 3x3x3 convolutions are variational-dropout layers (`nn.BayesConv3d`) when bayes=True —
the one model of the reference that yields an uncertainty estimate (sample the forward pass repeatedly).  Same attribute names
and state_dict keys (`init_conv`, `down1`..`down9`, `up1`..`up3`, `out`); the reference's file name starts with a digit and cannot
be imported as a module, this one is `bayes_unet`.

The reference's two-device split (`devices=[enc, dec]`) is not built: anything but None raises.
"""
import torch
import torch.nn as tnn

from ... import nn as mnn
from .bayes_layers import BasicDownBlock, BasicUpBlock


class UNet3D(tnn.Module):
    def __init__(self, n_classes, n_channels=[1, 16, 32, 64, 128], bayes=False, devices=None, shorten=False):
        super().__init__()
        if devices is not None:
            raise NotImplementedError("UNet3D(devices=...): the two-device split of the reference is not supported; use devices=None")
        self.bayes, self.devices, self.shorten = bayes, devices, shorten
        c = list(n_channels)
        first = mnn.BayesConv3d if bayes else mnn.Conv3d
        self.init_conv = first(c[0], c[1], kernel_size=3, padding=1, bias=False)
        plan = [(1, c[1], c[2], True), (2, c[2], c[2], False), (3, c[2], c[3], True), (4, c[3], c[3], False), (5, c[3], c[4], True),
                (6, c[4], c[4], False)]
        if not shorten:
            plan += [(i, c[4], c[4], False) for i in (7, 8, 9)]
        for i, cin, cout, down in plan:
            setattr(self, "down%d" % i, BasicDownBlock(cin, cout, downsample=down, bayes=bayes))
        self.n_down = len(plan)
        self.up1 = BasicUpBlock(c[4], c[3], bayes=bayes)
        self.up2 = BasicUpBlock(c[3], c[2], bayes=bayes)
        self.up3 = BasicUpBlock(c[2], c[1], bayes=bayes)
        self.out = mnn.Conv3d(c[1], n_classes, kernel_size=1, bias=False)

    def forward(self, x):
        x1 = self.init_conv(x)
        x2 = self.down2(self.down1(x1))
        x3 = self.down4(self.down3(x2))
        x4 = self.down5(x3)
        for i in range(6, self.n_down + 1):
            x4 = getattr(self, "down%d" % i)(x4)
        x4 = self.up1(x4, x3)
        x4 = self.up2(x4, x2)
        x4 = self.up3(x4, x1)
        return self.out(x4)

    def load_weights(self, base_file):
        """Strict-load a `.pth` / `.pkl` state_dict written by the reference model (or by this one)."""
        self.load_state_dict(torch.load(base_file, map_location="cpu", weights_only=True))
