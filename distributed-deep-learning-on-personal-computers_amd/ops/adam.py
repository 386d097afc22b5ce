"""Flat fused Adam (K14 of SURVEY.md §2.5).

Reference: ``torch.optim.Adam(model.parameters())`` at defaults (lr 1e-3, betas
(0.9, 0.999), eps 1e-8, no weight decay; ref.py:704), stepped on every rank with identical
gradients (ref.py:437,552).  The reference ships the live Adam object to the workers by
pickle (ref.py:561); here each rank builds its own from the same config.

Implementation: parameters, gradients and both moments live in flat fp32 buffers
(``parallel.flat.FlatParams``).  On GPU one HIP launch (``adam_step`` in
``csrc/misc.hip``) updates the whole model — 8.7 M elements, 4 streams read + 3 written,
HBM-bound — and, when a weight-pack table is attached, ALSO writes the bf16 copies of the
conv weights in the layouts the conv kernels consume (KRSC for forward, flipped CRSK for
dgrad), so no separate cast/transpose pass runs before the next forward.  On CPU the
same update is a handful of vectorised torch ops on the flat buffers.

``state_dict()`` is format-compatible with ``torch.optim.Adam`` (per-parameter ``step``,
``exp_avg``, ``exp_avg_sq``), so checkpoints load into either optimizer.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _ext


LR_SCHEDULES = ("constant", "poly", "cosine")       # sched_kind of adam_step_sched: the index


def grad_sqnorm_blocks(n: int) -> int:
    """Python twin of ``grad_sqnorm_blocks`` (csrc/optim.hip): the fp64 partial sums of the
    gradient norm, a function of ``n`` alone (``adam_step_sched`` refuses a shorter buffer)."""
    return 0 if n <= 0 else min(max((n // 4 + 255) // 256, 1), 1024)


def schedule_lr(t: int, lr: float, schedule: str = "constant", warmup: int = 0, total: int = 0,
                lr_min: float = 0.0, power: float = 0.9) -> float:
    """The learning rate of optimizer step ``t`` (1-based): the Python-double twin of ``sched_lr``
    (csrc/optim_math.h), operation for operation.  With ``s = t - 1`` steps taken: ``lr (s + 1) /
    warmup`` while ``s < warmup``; then ``u = clamp((s - warmup) / max(1, total - warmup), 0, 1)``
    and ``lr_min + (lr - lr_min) f(u)``, ``f`` = 1 (constant), ``(1 - u)^power`` (poly) or
    ``0.5 (1 + cos(pi u))`` (cosine); poly and cosine stay at ``lr_min`` after step ``total``."""
    s, W, T = float(t - 1), float(warmup), float(total)
    if s < W:
        return lr * (s + 1.0) / W
    u = min(max((s - W) / max(1.0, T - W), 0.0), 1.0)
    f = 1.0
    if schedule == "poly":
        f = 1.0 - u if power == 1.0 else (1.0 - u) ** power
    elif schedule == "cosine":
        f = 0.5 * (1.0 + math.cos(math.pi * u))
    if schedule != "constant" and u >= 1.0:
        f = 0.0
    return lr_min + (lr - lr_min) * f


class FlatAdam(torch.optim.Optimizer):
    """Flat Adam / AdamW.  With every scheduling argument at its default, ``step()`` is the plain
    Adam of ``adam_step_dev`` / ``adam_step``.  Otherwise it is ``adam_step_sched``
    (csrc/optim.hip, CPU twin in csrc/cpu_ref.cpp), all on the device and capturable:

    * ``lr_schedule`` ``constant | poly | cosine`` with ``warmup_steps`` of linear warm-up,
      ``total_steps``, ``lr_min`` and ``poly_power`` (``lr_at`` is the formula);
    * ``max_grad_norm > 0``: the flat gradient is scaled by ``min(max_norm / (norm + 1e-6), 1)``
      (``torch.nn.utils.clip_grad_norm_``) inside the update; the gradient buffer is not written;
    * ``decoupled=True``: ``p *= 1 - lr_t * weight_decay`` before the update (``torch.optim.AdamW``)
      in place of ``g += weight_decay * p``.

    A NaN / Inf gradient norm is not skipped: it propagates into every parameter, as in PyTorch.
    The schedule is a function of the step count alone, which ``load_state_dict`` restores, so a
    resumed run continues it; nothing else goes into the optimizer state."""

    def __init__(self, flat, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, use_hip: Optional[bool] = None, *,
                 decoupled: bool = False, max_grad_norm: float = 0.0,
                 lr_schedule: str = "constant", warmup_steps: int = 0, total_steps: int = 0,
                 lr_min: float = 0.0, poly_power: float = 0.9):
        if lr_schedule not in LR_SCHEDULES:
            raise ValueError(f"lr_schedule={lr_schedule!r} not in {LR_SCHEDULES}")
        if warmup_steps < 0 or total_steps < 0 or lr_min < 0 or max_grad_norm < 0:
            raise ValueError("warmup_steps, total_steps, lr_min and max_grad_norm must be >= 0")
        if lr_min > lr:
            raise ValueError("lr_min must not exceed lr")
        if poly_power <= 0:
            raise ValueError("poly_power must be > 0")
        # (total_steps may be set after construction — the Trainer derives it from its sampler)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None)
        self.flat = flat
        super().__init__(flat.params, defaults)
        dev = flat.param_buf.device
        self.exp_avg = torch.zeros_like(flat.param_buf)
        self.exp_avg_sq = torch.zeros_like(flat.param_buf)
        self.step_count = 0
        self._bind_state()
        self.weight_pack = None          # set by ops.fused_unet (bf16 conv-weight copies)
        self._dev_scal = None            # device [t, step_size, inv_sqrt_bc2] (hipGraph mode)
        self._use_hip = (dev.type == "cuda") if use_hip is None else use_hip
        self.decoupled, self.max_grad_norm = bool(decoupled), float(max_grad_norm)
        self.lr_schedule, self.warmup_steps = lr_schedule, int(warmup_steps)
        self.total_steps, self.lr_min, self.poly_power = int(total_steps), float(lr_min), float(poly_power)
        # any scheduling argument off its default: the adam_step_sched path on either device
        self.scheduled = bool(self.decoupled or self.max_grad_norm > 0 or lr_schedule != "constant"
                              or self.warmup_steps or self.total_steps or self.lr_min
                              or self.poly_power != 0.9)
        self._partial = None
        if self.scheduled:
            _ext.ops()                   # both devices run the kernel library's operator
            # the float[8] table of csrc/optim_math.h; [0] = steps taken (what _dev_scal[0] is)
            self._dev_scal = torch.zeros(8, dtype=torch.float32, device=dev)
            self._partial = torch.zeros(grad_sqnorm_blocks(flat.param_buf.numel()),
                                        dtype=torch.float64, device=dev)
        elif self._use_hip:
            _ext.ops()                   # fail loudly if the kernel library is missing
            # bias corrections on the device: identical arithmetic for eager and hipGraph
            # steps, and nothing step-dependent is baked into a captured graph
            self.enable_device_scalars()

    def _bind_state(self):
        for p in self.flat.params:
            a, b = self.flat.span(p)
            st = self.state[p]
            st["step"] = torch.tensor(float(self.step_count))
            st["exp_avg"] = self.flat._view(self.exp_avg, a, p)
            st["exp_avg_sq"] = self.flat._view(self.exp_avg_sq, a, p)

    def enable_device_scalars(self):
        """Bias corrections computed ON the device (adam_step_dev), so a captured step
        replays correctly: no host scalar is baked into the graph."""
        if not self._use_hip:
            raise RuntimeError("device-side Adam scalars need the HIP kernel library")
        if self.scheduled:
            return                       # (the scheduled step keeps all its scalars on the device)
        self._dev_scal = torch.tensor([float(self.step_count), 0.0, 0.0],
                                      dtype=torch.float32, device=self.flat.param_buf.device)

    def note_replayed_step(self):
        """Host mirror of a step executed by a graph replay."""
        self.step_count += 1

    def zero_grad(self, set_to_none: bool = False):
        self.flat.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        lr, (b1, b2), eps, wd = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        self.step_count += 1
        P, G = self.flat.param_buf, self.flat.grad_buf
        if self.scheduled:
            _ext.ops().adam_step_sched(P, G, self.exp_avg, self.exp_avg_sq, self._dev_scal,
                                       self._partial, float(lr), float(b1), float(b2), float(eps),
                                       float(wd), self.decoupled, self.max_grad_norm,
                                       LR_SCHEDULES.index(self.lr_schedule), self.warmup_steps,
                                       self.total_steps, self.lr_min, self.poly_power)
            if self.weight_pack is not None:
                self.weight_pack()
            return loss
        if self._dev_scal is not None:
            _ext.ops().adam_step_dev(P, G, self.exp_avg, self.exp_avg_sq, self._dev_scal,
                                     float(lr), float(b1), float(b2), float(eps), float(wd))
            if self.weight_pack is not None:
                self.weight_pack()
            return loss
        t = self.step_count
        bc1 = 1.0 - b1 ** t
        bc2 = 1.0 - b2 ** t
        step_size = lr / bc1
        inv_sqrt_bc2 = 1.0 / math.sqrt(bc2)
        if self._use_hip:
            _ext.ops().adam_step(P, G, self.exp_avg, self.exp_avg_sq, float(b1), float(b2),
                                 float(eps), float(wd), float(step_size), float(inv_sqrt_bc2))
            if self.weight_pack is not None:
                self.weight_pack()
        else:
            grad = G if wd == 0 else G.add(P, alpha=wd)
            self.exp_avg.lerp_(grad, 1.0 - b1)
            self.exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1.0 - b2)
            denom = (self.exp_avg_sq.sqrt() * inv_sqrt_bc2).add_(eps)
            P.addcdiv_(self.exp_avg, denom, value=-step_size)
        return loss

    def lr_at(self, t: int) -> float:
        """The learning rate of optimizer step ``t`` (1-based), as the device computes it."""
        return schedule_lr(t, float(self.param_groups[0]["lr"]), self.lr_schedule, self.warmup_steps,
                           self.total_steps, self.lr_min, self.poly_power)

    def last_stats(self):
        """``{lr, grad_norm, clip_coef}`` of the last scheduled step, read from the device table
        (synchronises; ``grad_norm`` is 0 with clipping off)."""
        if not self.scheduled:
            raise RuntimeError("last_stats: no schedule, clipping or decoupled decay is configured")
        s = self._dev_scal.tolist()
        return {"lr": s[3], "grad_norm": s[4], "clip_coef": s[5]}

    def _sync_steps(self):
        for p in self.flat.params:
            self.state[p]["step"].fill_(float(self.step_count))

    def state_dict(self):
        self._sync_steps()       # per-parameter step counters are refreshed lazily
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        steps = []
        with torch.no_grad():
            for p in self.flat.params:
                st = self.state.get(p, {})
                a, b = self.flat.span(p)
                if "exp_avg" in st:
                    self.flat._view(self.exp_avg, a, p).copy_(st["exp_avg"])
                    self.flat._view(self.exp_avg_sq, a, p).copy_(st["exp_avg_sq"])
                if "step" in st:
                    steps.append(int(float(st["step"])))
        self.step_count = max(steps) if steps else 0
        if self._dev_scal is not None:
            self._dev_scal[0] = float(self.step_count)
        self._bind_state()
        if self.weight_pack is not None:
            self.weight_pack()
