"""Gradient codec entry points (K16-K18 of SURVEY.md §2.5).

Three ``torch.ops.ddlpc`` operators, dispatched by tensor device: ``codec_absmax`` (one
multi-segment absmax pass, K16), ``codec_encode`` (quantise to fp16/int8 levels, K17) and
``codec_decode_sum`` (dequantise W payloads, weight and sum in rank order into the fp32
gradient, K18) — the fused HIP kernels of ``csrc/misc.hip`` for GPU tensors, the C++ kernels
of ``csrc/cpu_ref.cpp`` for CPU tensors.  ``parallel.codec`` is the torch oracle both are
tested against (same formulas, bit-exact rounding: round-half-to-even like torch.round).

Non-finite gradients are not hidden: a segment that holds a NaN gets the scale NaN, one that
holds an Inf the scale +Inf, its payload is zeros, and ``0 / L * scale`` decodes the whole
segment to NaN on every rank (tests/test_update_exact_gpu.py::test_codec_nonfinite).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from . import _ext

CODEC_ID = {"fp16_absmax": 0, "int8_absmax": 1}


def _seg_tensor(segments, device):
    return torch.tensor([x for s in segments for x in s], dtype=torch.int64, device=device)


def encode_segments(flat: torch.Tensor, segments: List[Tuple[int, int]], codec: str
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    ext = _ext.ops()
    seg = _seg_tensor(segments, flat.device)
    scales = ext.codec_absmax(flat, seg)
    payload = ext.codec_encode(flat, seg, scales, CODEC_ID[codec])
    return payload, scales


def decode_sum_segments(out: torch.Tensor, payloads: Sequence[torch.Tensor],
                        scales: Sequence[torch.Tensor], segments: List[Tuple[int, int]],
                        codec: str, weights: Sequence[float]):
    """out[seg] = sum_r weights[r] * decode(payloads[r][seg], scales[r][k])."""
    ext = _ext.ops()
    seg = _seg_tensor(segments, out.device)
    q = torch.stack(list(payloads))
    s = torch.stack(list(scales))
    w = torch.tensor(list(weights), dtype=torch.float32, device=out.device)
    ext.codec_decode_sum(out, q, s, w, seg, CODEC_ID[codec])
    return out


def topk_encode(g: torch.Tensor, residual: torch.Tensor, k: int
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k with error feedback on one bucket segment (``parallel.codec.topk_encode`` is the
    contract): ``residual += g``; the ``k`` largest magnitudes leave as ``(idx int32 ascending,
    val)`` and become +0.0 in the residual.  GPU: radix select + ordered compaction
    (csrc/topk.hip), no host read."""
    idx, val = _ext.ops().topk_encode(g, residual, k)
    return idx, val


def topk_decode_sum(out: torch.Tensor, idx: Sequence[torch.Tensor], val: Sequence[torch.Tensor],
                    weights: Sequence[float]):
    """out = sum_r weights[r] * val[r] scattered at idx[r], in rank order; the rest +0.0."""
    w = torch.tensor(list(weights), dtype=torch.float32, device=out.device)
    _ext.ops().topk_decode_sum(out, torch.stack(list(idx)), torch.stack(list(val)), w)
    return out


# Low-rank codec (``parallel.codec.powersgd_*`` is the contract; csrc/powersgd.hip).  ``low`` /
# ``raw`` are the plan's tables on the buffers' device; a caller passes the SAME table tensors on
# every call, so the GPU binding checks their values on the host once.  One launch per call.
def psgd_project(g, e, q, wire_p, low, raw, rank: int, w: float):
    """``e += g`` on the low-rank tensors, ``wire_p[P] = w (e q)``, ``wire_p[raw] = w g``."""
    _ext.ops().psgd_project(g, e, q, wire_p, low, raw, rank, w)


def psgd_orthonormalize(wire_p, low, rank: int):
    """Every ``P`` block of ``wire_p`` in place: modified Gram-Schmidt, fp64 sums."""
    _ext.ops().psgd_orthonormalize(wire_p, low, rank)


def psgd_backproject(e, wire_p, q_loc, wire_q, low, rank: int, w: float):
    """``q_loc = e^T P_hat``, ``wire_q = w q_loc``."""
    _ext.ops().psgd_backproject(e, wire_p, q_loc, wire_q, low, rank, w)


def psgd_residual(e, wire_p, q_loc, low, rank: int):
    """``e -= P_hat q_loc^T``."""
    _ext.ops().psgd_residual(e, wire_p, q_loc, low, rank)


def psgd_decode(g, wire_p, wire_q, low, raw, rank: int):
    """``g = P_hat Q^T`` on the low-rank tensors, ``g = wire_p[raw]`` on the raw spans."""
    _ext.ops().psgd_decode(g, wire_p, wire_q, low, raw, rank)
