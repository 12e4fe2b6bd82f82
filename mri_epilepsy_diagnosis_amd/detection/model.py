"""detection/model_utils.py:19-52 — PatchModel and ConvolutionBlock with the reference's constructors, forward and state_dict
(conv_blocks.{0..4}.conv.{weight,bias} with 4-D weights, conv_blocks.{0..4}.bn.*, fc1.*, fc2.*).

The five Conv2d -> BatchNorm2d -> ReLU blocks and the pool run on the HIP operators as one-slice volumes (N, C, 1, H, W):
`forward` lifts the (N, 2, 16, 32) batch once and the blocks hand the 5-D form on, so the fused BatchNorm + ReLU pass and the pool
serve them and nothing moves between layouts.  Flatten restores the reference's NCHW element order for fc1; Dropout, the two
Linear layers and the last ReLU work on (N, F) head vectors and stay torch's, as everywhere in this package."""
import torch
import torch.nn as tnn

from .. import nn


class ConvolutionBlock(tnn.Module):
    def __init__(self, in_c, out_c, pad=0):
        super().__init__()
        self.conv = nn.Conv2d(in_c, out_c, kernel_size=3, padding=pad)
        self.bn = nn.BatchNorm2d(out_c)
        self.relu = nn.ReLU()

    def forward(self, x):
        four = x.dim() == 4
        y = nn.fused_norm_act(self.bn, self.relu, self.conv(x.unsqueeze(2) if four else x))
        return y.squeeze(2) if four else y


class PatchModel(tnn.Module):
    def __init__(self):
        super().__init__()
        self.conv_blocks = tnn.Sequential(
            ConvolutionBlock(2, 16),
            ConvolutionBlock(16, 32),
            ConvolutionBlock(32, 64),
            ConvolutionBlock(64, 128),
            ConvolutionBlock(128, 256),
            nn.MaxPool2d(2)
        )
        self.flatten = nn.Flatten()
        self.dropout = tnn.Dropout(p=0.4)
        self.fc1 = tnn.Linear(3 * 11 * 256, 256)
        self.fc2 = tnn.Linear(256, 2)

    def forward(self, x):
        if x.dim() != 4:
            raise RuntimeError("PatchModel expects (N, 2, H, W) patches, got shape %s" % (tuple(x.shape),))
        x = self.conv_blocks(x.unsqueeze(2))
        x = self.flatten(x)
        x = self.dropout(x)
        x = torch.relu(self.fc1(x))
        x = self.fc2(x)
        return x
