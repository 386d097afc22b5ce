"""Lossy gradient codec (the reference's ``model_bytes`` compression, ref.py:25,328-545).

Reference formulas (bit-exact here):

* scale   ``max_grad = max over params of max|grad|``   (ref.py:328-340 / 451-463)
* encode  ``q = round(g / max_grad * L)`` cast to fp16 (L = 100) or int8 (L = 10)
          (ref.py:375 / 487 and ref.py:354 / 474)
* decode  ``q.float() / L * max_grad``                 (ref.py:304,313,426,430,533,543)

The reference sends per-tensor byte strings through pickle+mgzip to rank 0 which merges
and re-broadcasts (star).  Here every rank encodes its gradient bucket, the packed
payloads and scales are ``all_gather``-ed, and every rank decodes and sums them in rank
order -> all ranks get bit-identical gradients (the reference achieves that by making the
server also use the decoded copy, ref.py:402-433).

``scale`` granularity: ``global`` (reference parity: one scale over the whole gradient),
``bucket`` (default) or ``tensor``.  A global scale zeroes most small-magnitude tensors
(only 6.4 % non-zeros in fp16 mode on an init-time gradient).

The reference's ``float32`` mode is broken (NameError) and is not offered;
``grad_codec="none"`` is the lossless path.  An all-zero gradient (``max_grad == 0``), a
NameError in the reference, encodes to zeros here.

``grad_codec="topk"`` is not the reference's: top-k sparsification with error feedback (Deep
Gradient Compression / memory SGD).  Each rank keeps a residual, sends the ``k`` largest
magnitudes of ``residual + gradient`` per bucket as (index, value) pairs and keeps the rest for
the next exchange (``topk_encode`` / ``topk_decode_sum`` below; HIP kernels in csrc/topk.hip).

``grad_codec="powersgd"`` is the low-rank codec of Vogels et al. 2019 (PowerSGD) with error
feedback: every weight gradient, viewed as an ``n x m`` matrix, is sent as two thin factors that
are summed by plain all-reduces (``powersgd_plan`` and the five ``powersgd_*`` steps below; HIP
kernels in csrc/powersgd.hip).

On GPU the encode is ONE fused HIP kernel pass (absmax reduce + quantize; ``ops.codec``)
and the decode+sum another; this module is the torch oracle used on CPU and in tests.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

LEVELS = {"fp16_absmax": 100.0, "int8_absmax": 10.0}
WIRE_DTYPE = {"fp16_absmax": torch.float16, "int8_absmax": torch.int8}


def absmax(tensors: Sequence[torch.Tensor]) -> torch.Tensor:
    m = None
    for t in tensors:
        v = t.detach().abs().max().float()
        m = v if m is None else torch.maximum(m, v)
    return m


def encode(g: torch.Tensor, scale: torch.Tensor, codec: str) -> torch.Tensor:
    """round(g / scale * L) -> wire dtype.  scale == 0 encodes zeros."""
    L = LEVELS[codec]
    safe = torch.where(scale > 0, scale, torch.ones_like(scale))
    q = torch.round(g.float() / safe * L)
    q = torch.where(scale > 0, q, torch.zeros_like(q))
    return q.to(WIRE_DTYPE[codec])


def decode(q: torch.Tensor, scale: torch.Tensor, codec: str) -> torch.Tensor:
    L = LEVELS[codec]
    return q.to(torch.float32) / L * scale


def encode_segments(flat: torch.Tensor, segments: List[Tuple[int, int]], codec: str
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Encode a flat fp32 buffer with one absmax scale per ``(start, end)`` segment.
    Returns (payload in wire dtype, fp32 scales[len(segments)])."""
    scales = torch.stack([flat[a:b].abs().max().float() if b > a else
                          torch.zeros((), device=flat.device) for a, b in segments])
    out = torch.empty(flat.numel(), dtype=WIRE_DTYPE[codec], device=flat.device)
    for (a, b), s in zip(segments, scales):
        out[a:b] = encode(flat[a:b], s, codec)
    return out, scales


def decode_segments_accumulate(acc: torch.Tensor, q: torch.Tensor, scales: torch.Tensor,
                               segments: List[Tuple[int, int]], codec: str,
                               weight: float = 1.0):
    for (a, b), s in zip(segments, scales):
        acc[a:b] += decode(q[a:b], s, codec) * weight


def topk_count(n: int, ratio: float) -> int:
    """Entries sent of an ``n``-element bucket at ``ratio``: ``min(n, max(1, ceil(n * ratio)))``."""
    return min(n, max(1, math.ceil(n * ratio)))


def topk_encode(g: torch.Tensor, residual: torch.Tensor, k: int
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k sparsification with error feedback (``grad_codec="topk"``), the contract of the
    ``topk_encode`` operator.  ``a = residual + g`` (one fp32 add) replaces the residual;
    ``key = bits(a) & 0x7fffffff`` as an unsigned integer (every NaN above +Inf above every
    finite value, as for the absmax); ranked by key descending, then index ascending, the
    first ``k`` are sent as ``idx`` (int32, ascending) and ``val = a[idx]`` (bits kept) and
    become ``+0.0`` in the residual, which keeps everything that was not sent."""
    residual.add_(g)
    key = residual.view(torch.int32) & 0x7FFFFFFF              # non-negative: signed order = unsigned
    order = torch.sort(key, descending=True, stable=True).indices[:k]
    idx = torch.sort(order).values
    val = residual[idx].clone()
    residual[idx] = 0.0
    return idx.to(torch.int32), val


def topk_decode_sum(out: torch.Tensor, idx: Sequence[torch.Tensor], val: Sequence[torch.Tensor],
                    weights: Sequence[float]) -> torch.Tensor:
    """``out = sum over ranks r, in rank order, of weights[r] * val[r] scattered at idx[r]``:
    every element starts at +0.0, each rank adds ``fl(w * val)`` (two roundings, no fma),
    elements nobody sent stay +0.0."""
    out.zero_()
    for i, v, w in zip(idx, val, weights):
        out[i.long()] += v * torch.tensor(w, dtype=torch.float32, device=v.device)
    return out


# ---------------------------------------------------------------------------- low-rank codec
POWERSGD_MAX_RANK = 16


class PowerSGDPlan(NamedTuple):
    """The tables of one bucket (csrc/powersgd_math.h).  ``low`` int32 [T][5] = (offset in the
    bucket, n, m, p_off, q_off), ``raw`` int32 [R][3] = (offset, length, wire_off);
    ``wire_p = [raw values | P blocks, row-major n x r]`` and ``wire_q = [Q blocks, row-major
    m x r]`` are the sizes of the two wire buffers in floats; ``dense`` counts the bucket's
    parameter elements (the alignment gaps of the flat layout belong to nothing)."""
    rank: int
    low: torch.Tensor
    raw: torch.Tensor
    wire_p: int
    wire_q: int
    dense: int


def powersgd_plan(flat, params, start: int, rank: int) -> PowerSGDPlan:
    """Plan of the bucket that starts at ``start`` of the flat buffer and holds ``params`` (in
    ``flat.order``).  A parameter is low-rank iff ``p.dim() >= 2``, its flat view is contiguous
    and, with ``n = shape[0]`` and ``m = numel / n``, ``(n + m) r < n m`` (which implies
    ``r < min(n, m)``); everything else — biases, BatchNorm weights, tiny tensors — is raw.
    OIHW conv weights give ``Cout x (Cin 9)``, IOHW transposed-conv weights ``Cin x (Cout 4)``."""
    if not 1 <= rank <= POWERSGD_MAX_RANK:
        raise ValueError(f"powersgd_rank={rank!r} not in 1..{POWERSGD_MAX_RANK}")
    shapes, raws = [], []
    for p in params:
        a, b = flat.span(p)
        n = p.shape[0] if p.dim() >= 2 else 0
        m = p.numel() // n if n else 0
        if n and p.is_contiguous() and (n + m) * rank < n * m:
            shapes.append((a - start, n, m))
        elif b > a:
            raws.append((a - start, b - a))
    raw, wire = [], 0
    for off, length in raws:
        raw.append((off, length, wire))
        wire += length
    low, q_off = [], 0
    for off, n, m in shapes:
        low.append((off, n, m, wire, q_off))
        wire += n * rank
        q_off += m * rank
    return PowerSGDPlan(rank, torch.tensor(low, dtype=torch.int32).reshape(-1, 5),
                        torch.tensor(raw, dtype=torch.int32).reshape(-1, 3), wire, q_off,
                        sum(n * m for _, n, m in shapes) + sum(length for _, length in raws))


def powersgd_init_q(plan: PowerSGDPlan, seed: int, bucket: int) -> torch.Tensor:
    """The warm start ``q_prev`` of a bucket: standard normal fp32 from a CPU generator seeded by
    ``(seed, bucket index)``, so every rank and device starts from the same bits."""
    gen = torch.Generator().manual_seed((int(seed) * 1000003 + int(bucket)) % (1 << 63))
    return torch.randn(plan.wire_q, generator=gen, dtype=torch.float32)


def _low_rows(plan: PowerSGDPlan):
    return [tuple(int(v) for v in row) for row in plan.low.tolist()]


def powersgd_project(g, e, q, wire_p, plan: PowerSGDPlan, w: float):
    """Step 1.  Low-rank tensors: ``A = e + g`` (one add) written over ``e``, ``wire_p[P] =
    w (A q_prev)``; raw spans: ``wire_p[raw] = w g`` (their ``e`` is not touched: they are sent
    as they are).  Then ``all_reduce(SUM, wire_p)``.  These reference steps work in the dtype
    they are given (fp32 or fp64); the kernels accumulate the product in fp32."""
    r = plan.rank
    for off, n, m, po, qo in _low_rows(plan):
        a = e[off:off + n * m].add_(g[off:off + n * m]).view(n, m)
        wire_p[po:po + n * r] = (w * (a @ q[qo:qo + m * r].view(m, r))).reshape(-1)
    for off, length, wo in plan.raw.tolist():
        wire_p[wo:wo + length] = w * g[off:off + length]


def powersgd_orthonormalize(wire_p, plan: PowerSGDPlan):
    """Step 2.  Every reduced ``P`` in place, by modified Gram-Schmidt over its ``r`` columns: for
    column ``i``, ``s = 1 / sqrt(sum v_i^2)`` (the sum in double, ``s`` rounded once), ``q_i = s
    v_i``, then for every ``k > i``: ``d = sum q_i v_k`` (in double, rounded once) and ``v_k <-
    fma(-d, q_i, v_k)``.  A column whose squared norm is 0 becomes a zero column and contributes
    nothing.  NaN / Inf are not skipped: they propagate to the decoded gradient on every rank."""
    r, dt = plan.rank, wire_p.dtype
    for _, n, _, po, _ in _low_rows(plan):
        p = wire_p[po:po + n * r].view(n, r)
        for i in range(r):
            s2 = (p[:, i].double() ** 2).sum()
            p[:, i] = torch.zeros_like(p[:, i]) if float(s2) == 0.0 else p[:, i] * (1.0 / s2.sqrt()).to(dt)
            for k in range(i + 1, r):
                d = (p[:, i].double() * p[:, k].double()).sum().to(dt)
                p[:, k] = p[:, k] - d * p[:, i]


def powersgd_backproject(e, wire_p, q_loc, wire_q, plan: PowerSGDPlan, w: float):
    """Step 3.  ``Q_loc = A^T P_hat`` (``A`` in ``e`` since step 1), kept unscaled; ``wire_q = w
    Q_loc``.  Its ``all_reduce(SUM, wire_q)`` follows step 4."""
    r = plan.rank
    for off, n, m, po, qo in _low_rows(plan):
        ql = e[off:off + n * m].view(n, m).t() @ wire_p[po:po + n * r].view(n, r)
        q_loc[qo:qo + m * r] = ql.reshape(-1)
        wire_q[qo:qo + m * r] = w * ql.reshape(-1)


def _powersgd_pqt(p, q):
    """``P Q^T`` as the kernels' chain over ``j = 0 .. r - 1`` from 0 (theirs is an fma chain)."""
    acc = torch.zeros(p.shape[0], q.shape[0], dtype=p.dtype)
    for j in range(p.shape[1]):
        acc = acc + p[:, j, None] * q[None, :, j]
    return acc


def powersgd_residual(e, wire_p, q_loc, plan: PowerSGDPlan):
    """Step 4.  ``e <- A - P_hat Q_loc^T``: the part of this rank's ``A`` that THIS rank did not
    contribute.  This differs from the paper's ``A - decoded`` on purpose: with the local form
    ``sum_i w_i (A_i - e_i) = decoded`` holds by linearity for every reduce mode, the skewed
    ``reference`` weights included, so nothing is lost between the ranks' residuals and the
    decoded gradient.  For world size 1 the two forms coincide."""
    r = plan.rank
    for off, n, m, po, qo in _low_rows(plan):
        a = e[off:off + n * m].view(n, m)
        a -= _powersgd_pqt(wire_p[po:po + n * r].view(n, r), q_loc[qo:qo + m * r].view(m, r))


def powersgd_decode(g, wire_p, wire_q, plan: PowerSGDPlan):
    """Step 5.  ``g <- P_hat Q^T`` with the reduced ``Q`` on the low-rank tensors, ``g <-
    wire_p[raw]`` on the raw spans; the caller keeps the reduced ``Q`` as the next ``q_prev``.
    There is no re-seed: a tensor whose ``A`` is exactly zero on every rank in one exchange gets
    ``Q = 0``, so from then on ``P = A 0 = 0`` and the tensor is never sent again while its
    residual keeps every later gradient (a parameter without a gradient in some step — an unused
    branch — is such a tensor; rebuild the reducer to start it again)."""
    r = plan.rank
    for off, n, m, po, qo in _low_rows(plan):
        g[off:off + n * m] = _powersgd_pqt(wire_p[po:po + n * r].view(n, r),
                                           wire_q[qo:qo + m * r].view(m, r)).reshape(-1)
    for off, length, wo in plan.raw.tolist():
        g[off:off + length] = wire_p[wo:wo + length]


def reference_weights(world_size: int) -> List[float]:
    """Per-rank weights of the reference's "crooked averaging" (ref.py:268-315).

    Rank 0 divides its own grad by M once per worker message and adds each worker's
    decoded grad / M: final = g0 / M^M + sum_j q_j / M^(M-j+1), M = #workers
    (M=1 -> [1, 1] = a SUM; M=2 -> [1/4, 1/4, 1/2]).
    """
    M = world_size - 1
    if M <= 0:
        return [1.0]
    return [M ** (-M)] + [M ** (-(M - j + 1)) for j in range(1, M + 1)]


def relative_l2_error(g: torch.Tensor, codec: str, scale: Optional[torch.Tensor] = None
                      ) -> float:
    s = g.abs().max() if scale is None else scale
    r = decode(encode(g, s, codec), s, codec)
    return float((r - g).norm() / g.norm().clamp_min(1e-30))
