"""U-Net for semantic segmentation (2-D images or 3-D volumes).

Behavioural parity with the reference model (ref.py:575-656):

* ``DoubleConv``  = Conv(3, pad 1, bias) -> BN -> ReLU -> Conv -> BN -> ReLU held in
  ``self.double_conv`` as an ``nn.Sequential`` with indices 0..5 (ref.py:575-588).
* ``DownBlock``   returns ``(pooled, skip)`` with ``MaxPool(2)`` in ``down_sample``
  (ref.py:591-600).
* ``UpBlock``     ``up_sample`` is ``ConvTranspose(k2, s2)`` over ``in-out`` channels or a
  parameter-free bilinear x2 (align_corners=True); the up-sampled tensor comes FIRST in
  the channel concat (ref.py:603-617).
* ``UNet``        encoder widths ``(64,128,256,512,512) // width_divisor``, bottleneck
  ``double_conv``, decoder ``up_conv5..1`` and the 1x1 ``conv_last`` head
  (ref.py:620-656).  With depth=5 / dims=2 the ``state_dict`` has exactly the reference's
  166 keys (100 parameter tensors), so checkpoints interchange with the reference model.

Additions (BASELINE.json configs #1 and #5): ``depth`` (levels, 4 for the CPU plumbing
config) and ``dims`` (3 -> Conv3d/BatchNorm3d/MaxPool3d/ConvTranspose3d, trilinear).

Execution: on CPU (and for ``impl="torch"``) this module runs stock PyTorch layers — it is
the test oracle and the gloo plumbing path.  On an MI355X with ``impl="hip"`` the same
parameters are consumed by the hand-written HIP kernels in ``ops`` (NHWC bf16 implicit-GEMM
convolutions with fused BatchNorm/ReLU/max-pool/concat, fused head+cross-entropy); see
``ops/fused_unet.py``.  The public ``forward`` keeps the reference's NCHW float contract.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..config import ModelConfig


def _layers(dims: int):
    if dims == 2:
        return nn.Conv2d, nn.BatchNorm2d, nn.MaxPool2d, nn.ConvTranspose2d, "bilinear"
    if dims == 3:
        return nn.Conv3d, nn.BatchNorm3d, nn.MaxPool3d, nn.ConvTranspose3d, "trilinear"
    raise ValueError("dims must be 2 or 3")


class DoubleConv(nn.Module):
    """conv3 -> BN -> ReLU -> conv3 -> BN -> ReLU (ref.py:575-588)."""

    def __init__(self, in_channels: int, out_channels: int, dims: int = 2):
        super().__init__()
        Conv, BN, _, _, _ = _layers(dims)
        self.double_conv = nn.Sequential(
            Conv(in_channels, out_channels, kernel_size=3, padding=1),
            BN(out_channels),
            nn.ReLU(inplace=True),
            Conv(out_channels, out_channels, kernel_size=3, padding=1),
            BN(out_channels),
            nn.ReLU(inplace=True),
        )

    def forward(self, x):
        return self.double_conv(x)


class DownBlock(nn.Module):
    """DoubleConv then 2x max-pool; returns (down, skip) (ref.py:591-600)."""

    def __init__(self, in_channels: int, out_channels: int, dims: int = 2):
        super().__init__()
        _, _, Pool, _, _ = _layers(dims)
        self.double_conv = DoubleConv(in_channels, out_channels, dims)
        self.down_sample = Pool(2)

    def forward(self, x):
        skip_out = self.double_conv(x)
        down_out = self.down_sample(skip_out)
        return down_out, skip_out


class UpBlock(nn.Module):
    """Up-sample, concat([up, skip]), DoubleConv (ref.py:603-617)."""

    def __init__(self, in_channels: int, out_channels: int, up_sample_mode: str, dims: int = 2):
        super().__init__()
        _, _, _, ConvT, interp = _layers(dims)
        if up_sample_mode == "conv_transpose":
            self.up_sample = ConvT(in_channels - out_channels, in_channels - out_channels,
                                   kernel_size=2, stride=2)
        elif up_sample_mode == "bilinear":
            self.up_sample = nn.Upsample(scale_factor=2, mode=interp, align_corners=True)
        else:
            raise ValueError(
                "Unsupported `up_sample_mode` (can take one of `conv_transpose` or `bilinear`)")
        self.double_conv = DoubleConv(in_channels, out_channels, dims)

    def forward(self, down_input, skip_input):
        x = self.up_sample(down_input)
        x = torch.cat([x, skip_input], dim=1)
        return self.double_conv(x)


class UNet(nn.Module):
    """Reference-compatible U-Net (ref.py:620-656), generalised to depth/dims."""

    def __init__(self, out_classes: int = 2, up_sample_mode: str = "conv_transpose",
                 width_divisor: int = 2, depth: int = 5, dims: int = 2,
                 in_channels: int = 3, base_widths=(64, 128, 256, 512, 512)):
        super().__init__()
        cfg = ModelConfig(in_channels=in_channels, out_classes=out_classes,
                          width_divisor=width_divisor, depth=depth,
                          up_sample_mode=up_sample_mode, dims=dims,
                          base_widths=tuple(base_widths))
        cfg.validate()
        self.cfg = cfg
        self.up_sample_mode = up_sample_mode
        self.depth, self.dims = depth, dims
        e = cfg.widths()
        self.enc_widths = e
        Conv, _, _, _, _ = _layers(dims)
        prev = in_channels
        for i, w in enumerate(e):                       # down_conv1..depth
            setattr(self, f"down_conv{i + 1}", DownBlock(prev, w, dims))
            prev = w
        self.double_conv = DoubleConv(e[-1], e[-1], dims)  # bottleneck
        below = e[-1]
        for i in reversed(range(depth)):                # up_conv{depth}..1
            setattr(self, f"up_conv{i + 1}", UpBlock(below + e[i], e[i], up_sample_mode, dims))
            below = e[i]
        self.conv_last = Conv(e[0], out_classes, kernel_size=1)
        # Set by ops.fused_unet when the HIP path is attached (see ``to_hip``).
        self._engine = None

    @classmethod
    def from_config(cls, cfg: ModelConfig) -> "UNet":
        return cls(out_classes=cfg.out_classes, up_sample_mode=cfg.up_sample_mode,
                   width_divisor=cfg.width_divisor, depth=cfg.depth, dims=cfg.dims,
                   in_channels=cfg.in_channels, base_widths=cfg.base_widths)

    # ------------------------------------------------------------------ structure
    def down_blocks(self):
        return [getattr(self, f"down_conv{i + 1}") for i in range(self.depth)]

    def up_blocks(self):
        """Decoder blocks in execution order (deepest first)."""
        return [getattr(self, f"up_conv{i + 1}") for i in reversed(range(self.depth))]

    # ------------------------------------------------------------------ execution
    def forward(self, x):
        if self._engine is not None:
            return self._engine.forward(x)
        return self.forward_torch(x)

    def forward_torch(self, x):
        skips = []
        for blk in self.down_blocks():
            x, s = blk(x)
            skips.append(s)
        x = self.double_conv(x)
        for blk, s in zip(self.up_blocks(), reversed(skips)):
            x = blk(x, s)
        return self.conv_last(x)

    def loss_and_correct(self, x, y, ignore_index: int = -100, class_weight=None):
        """Mean cross-entropy (nn.CrossEntropyLoss defaults, ref.py:703) and the number of
        correctly classified pixels (ref.py:775).  The HIP path fuses the 1x1 head,
        softmax, CE, its gradient and the arg-max into one kernel (logits never hit HBM).

        ``class_weight`` (fp32 ``[out_classes]``, on the input's device) is
        ``CrossEntropyLoss(weight=...)``: the loss is ``sum w[y_p] ce_p / sum w[y_p]`` over the
        valid pixels; the hit count stays unweighted.  Where the weight sum is 0 (every pixel
        ignored, or every valid label of weight 0) the engine gives loss 0 and zero gradients;
        this stock path gives PyTorch's NaN."""
        if self._engine is not None:
            return self._engine.loss_and_correct(x, y, ignore_index, class_weight)
        logits = self.forward_torch(x)
        loss = F.cross_entropy(logits.float(), y, weight=class_weight, ignore_index=ignore_index)
        correct = (logits.detach().argmax(1) == y).sum()
        return loss, correct

    def to_hip(self, strict: bool = True):
        """Attach the operator engine (``ops.fused_unet.UNetEngine``; fails loudly if the kernel
        library is unavailable).  Its ``torch.ops.ddlpc`` calls run the hand-written gfx950
        kernels on GPU tensors and the C++ reference kernels on CPU tensors."""
        from ..ops.fused_unet import UNetEngine
        self._engine = UNetEngine(self, strict=strict)
        return self

    def detach_engine(self):
        self._engine = None
        return self
