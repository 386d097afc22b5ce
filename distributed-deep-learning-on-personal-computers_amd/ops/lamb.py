"""Flat LAMB (You et al. 2020, "Large Batch Optimization for Deep Learning"): Adam's moments with
one trust ratio ``||p_t|| / ||u_t||`` per parameter tensor, for the large-batch regime in which a
single global step size lets the wide and the narrow layers diverge.

``FlatLamb`` is ``FlatAdam``'s sibling on the same flat buffers: ``lamb_step`` (csrc/lamb.hip, CPU
twin in csrc/cpu_ref.cpp, the arithmetic in csrc/lamb_math.h) runs the whole step on the device —
schedule, warm-up and gradient-norm clipping as the scheduled Adam, then moments, per-tensor
norms, ratios and the update — with no host read, so a captured step replays correctly.  The
state is Adam's (``step``, ``exp_avg``, ``exp_avg_sq``): checkpoints load into either optimizer.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _ext
from .adam import LR_SCHEDULES, FlatAdam

LAMB_CHUNK = 1024            # kLambChunk of csrc/lamb_math.h


def lamb_tables(spans, adapted):
    """The chunk table and the tensor table of csrc/lamb_math.h for tensors at ``spans`` =
    ``[(begin, end)]`` (ascending, each begin a multiple of 4): int64 ``[C][3]`` = (tensor, begin,
    length) and ``[T][3]`` = (first chunk, chunk count, adapted flag).  A function of the layout
    alone."""
    chunks, tensors = [], []
    for t, ((a, b), flag) in enumerate(zip(spans, adapted)):
        if b <= a or a % 4:
            raise ValueError(f"tensor {t}: span ({a}, {b}) is empty or not 4-float aligned")
        first = len(chunks)
        chunks += [(t, o, min(LAMB_CHUNK, b - o)) for o in range(a, b, LAMB_CHUNK)]
        tensors.append((first, len(chunks) - first, int(bool(flag))))
    return (torch.tensor(chunks, dtype=torch.int64).reshape(-1, 3),
            torch.tensor(tensors, dtype=torch.int64).reshape(-1, 3))


class FlatLamb(FlatAdam):
    """Flat LAMB.  Per element of tensor ``t``, with the clipped gradient ``gc = g c``::

        m' = m + (1 - b1)(gc - m)        v' = b2 v + (1 - b2) gc gc
        r  = (m' / (1 - b1^t)) / (sqrt(v' / (1 - b2^t)) + eps)
        u  = r + weight_decay p          ratio_t = ||p_t|| / ||u_t||   (1 if either norm is 0)
        p' = p - lr_t ratio_t u

    The weight decay sits inside ``u`` (there is no coupled / decoupled choice).  With
    ``exclude_1d`` (the default) the 1-D parameters — biases, BatchNorm weights — get neither decay
    nor a trust ratio.  Schedule, warm-up and ``max_grad_norm`` are ``FlatAdam``'s arguments and
    mean the same; ``lr_at`` is the same formula.  The first step with a chunk table checks the
    table on the host, so one step must run before a capture (the trainer's warm-up steps do)."""

    def __init__(self, flat, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, use_hip: Optional[bool] = None, *, exclude_1d: bool = True,
                 max_grad_norm: float = 0.0, lr_schedule: str = "constant", warmup_steps: int = 0,
                 total_steps: int = 0, lr_min: float = 0.0, poly_power: float = 0.9):
        super().__init__(flat, lr, betas, eps, weight_decay, use_hip, max_grad_norm=max_grad_norm,
                         lr_schedule=lr_schedule, warmup_steps=warmup_steps, total_steps=total_steps,
                         lr_min=lr_min, poly_power=poly_power)
        _ext.ops()                       # both devices run the kernel library's operator
        self.scheduled = True            # (every scalar of a step lives in the device table)
        self.exclude_1d = bool(exclude_1d)
        dev = flat.param_buf.device
        self.adapted = [not (self.exclude_1d and p.dim() <= 1) for p in flat.order]
        chunks, tensors = lamb_tables([flat.span(p) for p in flat.order], self.adapted)
        self._chunks, self._tensors = chunks.to(dev), tensors.to(dev)
        # the float[8] table of csrc/lamb_math.h; [0] = steps taken
        self._dev_scal = torch.zeros(8, dtype=torch.float32, device=dev)
        self._partial = torch.zeros(3 * chunks.shape[0], dtype=torch.float64, device=dev)
        self.ratio = torch.ones(tensors.shape[0], dtype=torch.float32, device=dev)
        self.norms = torch.zeros(tensors.shape[0], 2, dtype=torch.float32, device=dev)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        (b1, b2) = g["betas"]
        self.step_count += 1
        _ext.ops().lamb_step(self.flat.param_buf, self.flat.grad_buf, self.exp_avg, self.exp_avg_sq,
                             self._dev_scal, self._chunks, self._tensors, self._partial, self.ratio,
                             self.norms, float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                             float(g["weight_decay"]), self.max_grad_norm,
                             LR_SCHEDULES.index(self.lr_schedule), self.warmup_steps, self.total_steps,
                             self.lr_min, self.poly_power)
        if self.weight_pack is not None:
            self.weight_pack()
        return loss

    def last_stats(self):
        """``{lr, grad_norm, clip_coef, trust_min, trust_max}`` of the last step, read from the
        device (synchronises); the trust ratios are those of the adapted tensors."""
        s = self._dev_scal.tolist()
        r = [x for x, a in zip(self.ratio.tolist(), self.adapted) if a] or [1.0]
        return {"lr": s[3], "grad_norm": s[4], "clip_coef": s[5], "trust_min": min(r), "trust_max": max(r)}
