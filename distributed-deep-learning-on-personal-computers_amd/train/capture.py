"""Captured micro-batches: static input buffers, and one "eager for ``warmup`` uses, then
capture, then replay" rule over them (the single-stream "acc" / "last" hipGraphs and the
per-stream graphs of the concurrent micro-batches both go through it).

A graph reads the static buffers it was captured over.  ``StaticInputs`` reallocates them
when the label shape changes (a short last batch) and counts that in ``version``; a
``CapturedMicro`` whose buffers were replaced drops its graph and warms up again.
"""
from __future__ import annotations

import torch

from ..data.datasets import engine_input


class StaticInputs:
    """One pair of static input buffers; several graphs may share it (replays that follow
    each other on one stream)."""

    def __init__(self):
        self.bufs = None
        self.version = 0                 # bumped whenever the buffers are replaced

    def stage(self, x: torch.Tensor, y: torch.Tensor):
        """Copy a micro-batch in (on the current stream) -> the static (x, y).  A
        device-pipeline batch (padded channel-last bf16, ``data.engine_input``) is copied in
        that layout, so a captured forward reads it with no layout pass."""
        xp = getattr(x, "_ddlpc_nhwc", None)
        if self.bufs is None or self.bufs[1].shape != y.shape:
            if xp is not None:
                sp = torch.empty_like(xp)
                self.bufs = (engine_input(sp, x.shape[1]), torch.empty_like(y), sp)
            else:
                self.bufs = (torch.empty_like(x), torch.empty_like(y), None)
            self.version += 1
        sx, sy, sp = self.bufs
        if sp is not None and xp is not None:
            sp.copy_(xp)
        else:
            sx.copy_(x)
        sy.copy_(y)
        return sx, sy


def on_fresh_stream(fn, device=None):
    """Run ``fn`` on a new side stream that waits on, and is waited for by, the current one."""
    cur = torch.cuda.current_stream(device)
    side = torch.cuda.Stream(device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        fn()
    cur.wait_stream(side)


def capture_graph(fn, stream=None, before=None):
    """``fn`` captured (not executed) into a new graph, on ``stream`` or torch's capture
    stream; ``before`` runs first, outside the capture."""
    if before is not None:
        before()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        fn()
    return g


class CapturedMicro:
    """``body(x, y)`` over ``static``: the first ``warmup`` calls run it through ``eager``
    (allocator and lazy-state warm-up), the last of them is followed by ``capture`` (which
    executes nothing), later calls replay.  ``eager`` / ``capture`` are the warm-up policy."""

    def __init__(self, static: StaticInputs, body, warmup: int, eager=lambda fn: fn(),
                 capture=capture_graph):
        self.static, self.body, self.warmup = static, body, warmup
        self.eager, self.capture = eager, capture
        self.graph, self.warm, self.version = None, 0, static.version

    def __call__(self, x: torch.Tensor, y: torch.Tensor) -> str:
        """Stage the batch and run it; -> what was done: "eager", "capture" (eager, then
        captured) or "replay"."""
        sx, sy = self.static.stage(x, y)
        if self.version != self.static.version:      # captured over buffers since replaced
            self.graph, self.warm, self.version = None, 0, self.static.version
        if self.graph is not None:
            self.graph.replay()
            return "replay"
        self.eager(lambda: self.body(sx, sy))
        self.warm += 1
        if self.warm < self.warmup:
            return "eager"
        self.graph = self.capture(lambda: self.body(sx, sy))
        return "capture"
