"""Label distance transform and boundary erosion (``csrc/boundary.hip``, CPU twin in
``csrc/cpu_ref.cpp``, the recipe in ``csrc/label_math.h``).

The ISPRS Vaihingen / Potsdam benchmark scores a second sheet, "eroded boundaries", that leaves out
every pixel within 3 px of a class border (the reference labels are unreliable there); published
figures are almost always of that kind.  Labels here are cut and resampled on the device, so the
band is computed on the device too: ``erode_labels`` rewrites it to the ignore value in front of the
unchanged head, evaluation and scene kernels, which skip ignored pixels.

Two ``torch.ops.ddlpc`` operators, dispatched by tensor device, one launch each, no host read:

* ``label_dist2(labels, K, ignore_index)`` -> int32, the squared Euclidean distance of every valid
  pixel (``0 <= l < K``, ``l != ignore_index``) to the nearest valid pixel of another class in the
  same image, truncated at 16 px (257 = none within 16; an invalid pixel has 0);
* ``label_erode(labels, K, ignore_index, radius, fill)`` -> the labels with every valid pixel at
  ``d2 <= radius**2`` rewritten to ``fill``.

``labels``: int64 ``[B, H, W]`` or uint8 ``[H, W]`` / ``[B, H, W]``, contiguous.
"""
from __future__ import annotations

import torch

from . import _ext

MAX_RADIUS = 16


def label_dist2(labels: torch.Tensor, classes: int, ignore_index: int = -100) -> torch.Tensor:
    return _ext.ops().label_dist2(labels.contiguous(), classes, ignore_index)


def erode_labels(labels: torch.Tensor, classes: int, radius: int, ignore_index: int = -100,
                 fill=None) -> torch.Tensor:
    """``labels`` with the boundary band of ``radius`` pixels rewritten to ``fill`` (default: the
    ignore value, 255 for uint8 labels).  ``radius = 0`` returns ``labels`` itself: no launch."""
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"erosion radius must be in 0..{MAX_RADIUS}, got {radius}")
    if radius == 0:
        return labels
    if fill is None:
        fill = 255 if labels.dtype == torch.uint8 else ignore_index
    return _ext.ops().label_erode(labels.contiguous(), classes, ignore_index, radius, fill)
