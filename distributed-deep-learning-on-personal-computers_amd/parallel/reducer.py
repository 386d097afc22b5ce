"""Bucketed data-parallel gradient reducer, overlapped with backward.

Replaces the reference's star exchange: workers encode
their accumulated gradients, send them to rank 0 over TCP, rank 0 merges, re-encodes and
sends back, everyone steps Adam (ref.py:255-556).  That serialises a 2*M*msg transfer
through one link and round-trips every tensor through the host.

MI355X design:

* gradients are views into ONE flat fp32 buffer (``FlatParams``); buckets are contiguous
  slices of it in backward order, sized by ``bucket_mb`` (few, large: on 7 point-to-point
  xGMI links per GPU a ring all-reduce is per-link bound, and per-collective latency is
  tens of µs, so 3-5 buckets of ~8 MB beat many small ones);
* ``register_post_accumulate_grad_hook`` marks parameters ready; when the LAST
  micro-batch's backward completes a bucket, its collective is launched immediately
  (async) so it runs on RCCL's own stream while backward continues on the compute
  stream: the deep decoder/bottleneck gradients (most of the bytes) reduce while the
  high-resolution encoder layers are still in backward;
* accumulation micro-batches (``frequency_sending_gradients``, ref.py:685/759) launch
  nothing (no_sync semantics);
* ``finish()`` makes the compute stream wait for every bucket (no host sync) before the
  optimizer step;
* reduction: correct mean (pre-scaled by 1/W, then SUM), ``sum``, or ``reference`` (the
  reference's skewed weights; for W=2 that is a plain sum);
* optional lossy codec (fp16/int8 absmax, ref.py:25) as an all-gather of packed payloads
  + scales, decoded and summed in rank order (``parallel.codec``; fused HIP kernels on GPU);
* optional top-k sparsification with error feedback (``grad_codec="topk"``): a flat fp32
  residual the size of the gradient buffer; per bucket ``topk_encode`` adds the gradient into
  its residual slice and takes the k = ``topk_ratio`` * n largest magnitudes out of it as
  (index, value) pairs — 8 bytes per sent entry on the wire — which are all-gathered and
  scatter-summed in rank order at ``finish()`` (csrc/topk.hip); what was not sent stays in the
  residual for the next exchange.  The residual is not checkpointed: a resume starts from zero;
* optional low-rank codec with error feedback (``grad_codec="powersgd"``, Vogels et al. 2019):
  every weight gradient of a bucket, viewed as an n x m matrix, travels as two thin factors
  P (n x r) and Q (m x r), r = ``powersgd_rank``, summed by two plain all-reduces — the cost per
  rank does not grow with the world size; biases and BatchNorm weights ride along as they are.
  The first all-reduce (P) is launched from backward, ``finish()`` orthonormalises P, forms Q and
  the residual and launches every bucket's second all-reduce before it waits for the first of
  them (csrc/powersgd.hip; the contract is ``parallel.codec.powersgd_*``).  The residual and
  the warm start ``q_prev`` are not checkpointed: a resume restarts both.  ``q_prev`` is never
  re-seeded: a weight whose residual + gradient is exactly zero on every rank in one exchange
  gets Q = 0 and is not sent again (``parallel.codec.powersgd_decode``);
* optional bf16 wire format (``wire_dtype="bf16"``): half the bytes of the fp32
  all-reduce — an all-to-all of bf16 chunks (the reduce-scatter's transport) launched
  asynchronously from backward, then in ``finish()`` a rank-ordered fp32 sum of the owned
  chunk and an all-gather of the sums.  LOSSY: each rank's gradient is rounded to bf16
  before the exchange and the reduced gradient is rounded to bf16 again before it is
  copied back into the fp32 grad buffer (every rank receives identical bits).  For slow
  links (the reference's "PCs over Ethernet" setting) this halves the bytes on the wire.
"""
from __future__ import annotations

import contextlib
from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist

from . import codec as C
from .flat import FlatParams


class _Bucket:
    __slots__ = ("idx", "start", "end", "params", "pending", "work", "payload", "scales",
                 "gathered", "launched", "wire", "ev", "psgd")

    def __init__(self, idx, start, end, params):
        self.idx, self.start, self.end, self.params = idx, start, end, params
        self.pending = len(params)
        self.work = None
        self.payload = self.scales = self.gathered = None
        self.launched = False
        self.wire = None                 # bf16 wire buffers (send, recv, owned chunk, out)
        self.ev = None                   # comm proxy: (ready, start, end) events
        self.psgd = None                 # low-rank codec: plan, tables and buffers


class _PowerSGDState:
    """Per bucket: the plan, its tables on the gradient's device, the two wire buffers, the
    warm start ``q_prev`` and this rank's ``q_loc`` (made on first use; gloo with GPU tensors:
    host copies of the wire buffers too)."""
    __slots__ = ("plan", "low", "raw", "wire_p", "wire_q", "q_prev", "q_loc", "host_p", "host_q")

    def __init__(self, plan):
        self.plan = plan
        self.low = self.raw = self.wire_p = self.wire_q = self.q_prev = self.q_loc = None
        self.host_p = self.host_q = None


class GradBucketReducer:
    def __init__(self, flat: FlatParams, group=None, bucket_mb: float = 8.0,
                 reduce: str = "mean", grad_codec: str = "none", codec_scale: str = "bucket",
                 overlap: bool = True, use_hooks: bool = True, wire_dtype: str = "fp32",
                 proxy: int = 0, cuts: Optional[List[int]] = None, topk_ratio: float = 0.01,
                 powersgd_rank: int = 4, powersgd_seed: int = 0):
        if wire_dtype not in ("fp32", "bf16"):
            raise ValueError(f"wire_dtype={wire_dtype!r}")
        if grad_codec == "topk" and (codec_scale != "bucket" or wire_dtype != "fp32"):
            raise ValueError("grad_codec='topk' needs codec_scale='bucket' and wire_dtype='fp32'")
        if not 0.0 < topk_ratio <= 1.0:
            raise ValueError(f"topk_ratio={topk_ratio!r} not in (0, 1]")
        if grad_codec == "powersgd" and (codec_scale != "bucket" or wire_dtype != "fp32"):
            raise ValueError("grad_codec='powersgd' needs codec_scale='bucket' and wire_dtype='fp32'")
        if not 1 <= powersgd_rank <= C.POWERSGD_MAX_RANK:
            raise ValueError(f"powersgd_rank={powersgd_rank!r} not in 1..{C.POWERSGD_MAX_RANK}")
        self.powersgd_rank, self.powersgd_seed = int(powersgd_rank), int(powersgd_seed)
        self.topk_ratio = topk_ratio
        self.residual: Optional[torch.Tensor] = None    # topk / powersgd error feedback, made on first use
        self.flat = flat
        self.wire_dtype = wire_dtype
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.backend = dist.get_backend(group) if dist.is_initialized() else None
        # comm proxy (single GPU; ``proxy`` = the world size it stands in for): every
        # bucket's collective is replaced by ``comm_proxy`` — 16 streaming workgroups (an
        # RCCL-like channel count) sweeping the bucket twice (reduce-scatter + all-gather
        # passes, values unchanged) — on a dedicated comm stream, launched at the same
        # readiness points as the real collective.  It measures how fast a collective
        # launched mid-backward gets CUs next to the persistent kernels.
        self.proxy = int(proxy) if self.world == 1 else 0
        self.proxy_stream = None
        self.proxy_log: List[Tuple[int, float, float]] = []
        if self.proxy:
            if grad_codec != "none" or wire_dtype != "fp32":
                raise ValueError("comm proxy: plain fp32 all-reduce only")
            self.world = 2                       # every rank path below behaves as DP ...
            reduce = "sum"                       # ... with the identity as the reduction
            self.proxy_stream = torch.cuda.Stream(flat.grad_buf.device)
        self.reduce, self.codec, self.codec_scale = reduce, grad_codec, codec_scale
        self.overlap = overlap and not (grad_codec != "none" and codec_scale == "global")
        if reduce == "mean":
            self.weight = 1.0 / self.world
        elif reduce == "sum":
            self.weight = 1.0
        elif reduce == "reference":
            self.weight = C.reference_weights(self.world)[self.rank]
        else:
            raise ValueError(reduce)
        # cuts: bucket boundaries as indices into flat.order (``parallel.bucket_plan``, the
        # readiness-aware plan); None = cut by size only
        self.cuts = list(cuts) if cuts is not None else None
        self.buckets = self._make_buckets(bucket_mb)
        self._bucket_of: Dict[int, _Bucket] = {}
        for b in self.buckets:
            for p in b.params:
                self._bucket_of[id(p)] = b
        # readiness is armed explicitly per accumulation window: only ``prepare(sync=True)``
        # (the window's last micro-batch) arms it and ``finish()`` disarms it, so a fresh
        # reducer — or one between windows — never launches a collective on a partially
        # accumulated gradient (ref.py:756-766: no exchange until the 50th micro-batch)
        self._sync = False
        self._seen = set()
        self._hooks = []
        # readiness: autograd post-accumulate hooks (stock PyTorch modules), or — with
        # use_hooks=False — ONLY explicit mark_ready() calls from kernels that write .grad
        # directly (the HIP engine).  Never both: autograd still runs the AccumulateGrad
        # nodes of such parameters (with no gradient), which would count them twice and
        # launch a bucket before its last gradient is written.
        if self.world > 1 and use_hooks and not self.proxy:
            for p in flat.order:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad_ready))
        self.stats = {"buckets": len(self.buckets), "launched_in_backward": 0}
        if grad_codec == "topk":                 # entries sent per exchange, over all buckets
            self.stats["topk_k"] = sum(C.topk_count(b.end - b.start, topk_ratio)
                                       for b in self.buckets)
        if grad_codec == "powersgd":             # floats on the wire per exchange and rank, over all buckets
            for b in self.buckets:
                b.psgd = _PowerSGDState(C.powersgd_plan(flat, b.params, b.start, self.powersgd_rank))
            self.stats["powersgd_wire_floats"] = sum(b.psgd.plan.wire_p + b.psgd.plan.wire_q
                                                     for b in self.buckets)
            self.stats["powersgd_dense_floats"] = sum(b.psgd.plan.dense for b in self.buckets)
        # readiness calibration (``start_calibration``): per-parameter gradient-complete times
        # of one synchronised step, relative to its backward start (Trainer.calibrate_bucket_plan)
        self._index = {id(p): i for i, p in enumerate(flat.order)}
        self._calib: Optional[Dict] = None
        self._bwd_start = None

    # ------------------------------------------------------------------ timing marks
    def _now(self):
        """A timing mark on the current stream (hipEvent), or the host clock on CPU (gloo: hooks
        fire synchronously on the host)."""
        dev = self.flat.grad_buf.device
        if dev.type == "cuda":
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(dev))
            return e
        import time
        return time.perf_counter()

    @staticmethod
    def _ms(a, b) -> float:
        return a.elapsed_time(b) if isinstance(a, torch.cuda.Event) else (b - a) * 1e3

    def mark_backward_start(self):
        """Called right before the synchronised micro-batch's backward is queued (its forward
        kernels are ahead of it on the stream): the zero of the readiness times."""
        if self._sync and (self._calib is not None or self.proxy):
            self._bwd_start = self._now()

    def start_calibration(self):
        self._calib = {"ready": {}, "end": None}

    def stop_calibration(self) -> Tuple[List[float], float]:
        """-> (ready ms of every parameter in flat order, backward ms) of the calibrated step,
        both measured from the backward start (synchronises).  A parameter never reported ready
        counts as ready at the backward's end."""
        cal, self._calib = self._calib, None
        if cal is None or self._bwd_start is None or cal["end"] is None:
            raise RuntimeError("calibration: no synchronised step was recorded")
        t0 = self._bwd_start
        if isinstance(t0, torch.cuda.Event):
            cal["end"].synchronize()
        bwd = self._ms(t0, cal["end"])
        ready = [bwd] * len(self.flat.order)
        for i, ev in cal["ready"].items():
            ready[i] = min(bwd, max(0.0, self._ms(t0, ev)))
        return ready, bwd

    # ------------------------------------------------------------------ setup
    def _make_buckets(self, bucket_mb: float) -> List[_Bucket]:
        order = self.flat.order
        if self.cuts is not None:
            c = self.cuts
            if c[0] != 0 or c[-1] != len(order) or any(b <= a for a, b in zip(c[:-1], c[1:])):
                raise ValueError(f"bucket cuts {c} do not partition {len(order)} parameters")
            out = []
            for a, b in zip(c[:-1], c[1:]):
                ps = order[a:b]
                out.append(_Bucket(len(out), self.flat.span(ps[0])[0], self.flat.span(ps[-1])[1], ps))
            return out
        cap = max(1, int(bucket_mb * (1 << 20) // 4))
        buckets, cur, start = [], [], None
        end = 0
        for p in self.flat.order:
            a, b = self.flat.span(p)
            if start is None:
                start = a
            if cur and (b - start) > cap:
                buckets.append(_Bucket(len(buckets), start, end, cur))
                cur, start = [], a
            cur.append(p)
            end = b
        if cur:
            buckets.append(_Bucket(len(buckets), start, end, cur))
        # last bucket extends over trailing alignment padding (harmless zeros)
        return buckets

    def bucket_ranges(self) -> List[Tuple[int, int]]:
        return [(b.start, b.end) for b in self.buckets]

    # ------------------------------------------------------------------ per step
    @contextlib.contextmanager
    def no_sync(self):
        prev, self._sync = self._sync, False
        try:
            yield
        finally:
            self._sync = prev

    def prepare(self, sync: bool = True):
        """Call before each micro-batch backward: ``sync`` only on the last one of the
        accumulation window (arms the bucket launches; ``finish()`` disarms them)."""
        self._sync = sync
        if sync:
            self._seen = set()
            for b in self.buckets:
                b.pending = len(b.params)
                b.work = None
                b.launched = False
                b.payload = b.scales = b.gathered = None

    def mark_ready(self, p):
        """Readiness notification from kernels that write .grad directly (HIP engine)."""
        self._on_grad_ready(p)

    def _on_grad_ready(self, p):
        if not self._sync or not self.overlap:
            return
        b = self._bucket_of.get(id(p))
        if b is None or id(p) in self._seen:       # a parameter counts once per step
            return
        self._seen.add(id(p))
        if self._calib is not None:
            self._calib["ready"][self._index[id(p)]] = self._now()
        b.pending -= 1
        if b.pending == 0 and not b.launched:
            self._launch(b)
            self.stats["launched_in_backward"] += 1

    def _seg(self, b: _Bucket) -> torch.Tensor:
        return self.flat.grad_buf[b.start:b.end]

    def _launch(self, b: _Bucket):
        b.launched = True
        g = self._seg(b)
        if self.proxy:
            self._launch_proxy(b, g)
            return
        if self.codec == "none":
            # pre-scaled SUM on every backend (exact for power-of-two world sizes; no
            # dependence on the collective library's AVG support)
            if self.weight != 1.0:
                g.mul_(self.weight)
            if self.wire_dtype == "bf16":
                self._launch_bf16(b, g)
                return
            b.work = dist.all_reduce(g, group=self.group, async_op=True)
            return
        # lossy codec: encode -> all_gather(payload, scales) -> decode+sum at finish()
        from ..ops import codec_ops
        if self.codec == "powersgd":
            # step 1: e <- e + g, wire_p = w (e q_prev) | w g[raw]; its all-reduce runs under backward
            st = self._psgd_buffers(b)
            codec_ops.psgd_project(g, self.residual[b.start:b.end], st.q_prev, st.wire_p, st.low, st.raw,
                                   self.powersgd_rank, self.weight)
            b.work = ("psgd", self._psgd_all_reduce(st.wire_p, st.host_p))
            return
        if self.codec == "topk":
            # (payload, scales) = (idx, val) of the k entries taken out of residual + gradient
            if self.residual is None:
                self.residual = torch.zeros_like(self.flat.grad_buf)
            k = C.topk_count(g.numel(), self.topk_ratio)
            b.payload, b.scales = codec_ops.topk_encode(g, self.residual[b.start:b.end], k)
            if self.backend == "gloo" and g.is_cuda:
                # gloo is a host transport: it gets host tensors (GPU tensors are for RCCL)
                b.payload, b.scales = b.payload.cpu(), b.scales.cpu()
        else:
            segs = self._codec_segments(b)
            b.payload, b.scales = codec_ops.encode_segments(g, segs, self.codec)
        b.gathered = ([torch.empty_like(b.payload) for _ in range(self.world)],
                      [torch.empty_like(b.scales) for _ in range(self.world)])
        w1 = dist.all_gather(b.gathered[0], b.payload, group=self.group, async_op=True)
        w2 = dist.all_gather(b.gathered[1], b.scales, group=self.group, async_op=True)
        b.work = (w1, w2)

    def _psgd_buffers(self, b: _Bucket) -> _PowerSGDState:
        st, dev = b.psgd, self.flat.grad_buf.device
        if st.wire_p is None:
            if self.residual is None:
                self.residual = torch.zeros_like(self.flat.grad_buf)
            st.low, st.raw = st.plan.low.to(dev), st.plan.raw.to(dev)
            st.wire_p = torch.zeros(st.plan.wire_p, dtype=torch.float32, device=dev)
            st.wire_q = torch.zeros(st.plan.wire_q, dtype=torch.float32, device=dev)
            st.q_loc = torch.zeros_like(st.wire_q)
            st.q_prev = C.powersgd_init_q(st.plan, self.powersgd_seed, b.idx).to(dev)
            if self.backend == "gloo" and dev.type == "cuda":
                # gloo is a host transport: it gets host tensors (GPU tensors are for RCCL)
                st.host_p = torch.empty(st.plan.wire_p, dtype=torch.float32, pin_memory=True)
                st.host_q = torch.empty(st.plan.wire_q, dtype=torch.float32, pin_memory=True)
        return st

    def _psgd_all_reduce(self, wire: torch.Tensor, host: Optional[torch.Tensor]):
        """-> (work, host copy or None) of the asynchronous SUM of one wire buffer."""
        if host is not None:
            host.copy_(wire)
            return dist.all_reduce(host, group=self.group, async_op=True), host
        return dist.all_reduce(wire, group=self.group, async_op=True), None

    @staticmethod
    def _psgd_wait(work, wire: torch.Tensor):
        w, host = work
        w.wait()
        if host is not None:
            wire.copy_(host)

    def _finish_powersgd(self):
        """Steps 2-4 of every bucket and its second all-reduce, and only then the waits and the
        decodes: the second round of collectives overlaps across the buckets."""
        from ..ops import codec_ops
        r = self.powersgd_rank
        for b in self.buckets:
            st, e = b.psgd, self.residual[b.start:b.end]
            self._psgd_wait(b.work[1], st.wire_p)
            codec_ops.psgd_orthonormalize(st.wire_p, st.low, r)
            codec_ops.psgd_backproject(e, st.wire_p, st.q_loc, st.wire_q, st.low, r, self.weight)
            codec_ops.psgd_residual(e, st.wire_p, st.q_loc, st.low, r)
            b.work = ("psgd", self._psgd_all_reduce(st.wire_q, st.host_q))
        for b in self.buckets:
            st = b.psgd
            self._psgd_wait(b.work[1], st.wire_q)
            codec_ops.psgd_decode(self._seg(b), st.wire_p, st.wire_q, st.low, st.raw, r)
            st.q_prev, st.wire_q = st.wire_q, st.q_prev       # the reduced Q is the next warm start
            b.work = None

    PROXY_BLOCKS = 16                    # RCCL-like channel count

    def _launch_proxy(self, b: _Bucket, g: torch.Tensor):
        cur = torch.cuda.current_stream(g.device)
        if b.ev is None:
            b.ev = tuple(torch.cuda.Event(enable_timing=True) for _ in range(3))
        ready, start, end = b.ev
        ready.record(cur)                    # gradients complete on the producing stream
        st = self.proxy_stream
        st.wait_stream(cur)                  # as RCCL's stream waits on the caller's
        with torch.cuda.stream(st):
            start.record(st)
            from ..ops import _ext
            # two sweeps: the reduce-scatter's and the all-gather's pass over the bucket
            _ext.ops().comm_proxy(g, self.PROXY_BLOCKS, 2)
            end.record(st)
        b.work = ("proxy", end)

    def proxy_times(self) -> List[Dict[str, float]]:
        """Per bucket of the last synchronised step: ms from gradients-ready to the proxy
        collective's start and end (synchronises on the events)."""
        out = []
        for b in self.buckets:
            if b.ev is None:
                continue
            ready, start, end = b.ev
            end.synchronize()
            rec = {"bucket": b.idx, "mb": round((b.end - b.start) * 4 / 2**20, 2),
                   "ready_to_start_ms": ready.elapsed_time(start),
                   "ready_to_end_ms": ready.elapsed_time(end),
                   "kernel_ms": start.elapsed_time(end)}
            if isinstance(self._bwd_start, torch.cuda.Event):
                # bucket collective end measured from the backward start (the plan's zero)
                rec["end_from_backward_start_ms"] = self._bwd_start.elapsed_time(end)
            bwd = getattr(self, "_bwd_end", None)
            if bwd is not None:
                bwd.synchronize()
                # > 0: the bucket's collective ended after backward (exposed)
                rec["end_after_backward_ms"] = bwd.elapsed_time(end)
            out.append(rec)
        return out

    def _launch_bf16(self, b: _Bucket, g: torch.Tensor):
        """bf16 transport, first half: the all-to-all of bf16 chunks, left in flight (its
        wait, the fp32 rank-order sum and the all-gather run in ``finish()``, so backward is
        never blocked by the exchange — on gloo a wait here would stall the host)."""
        n, W = g.numel(), self.world
        chunk = -(-n // W)
        if b.wire is None:
            send = torch.zeros(chunk * W, dtype=torch.bfloat16, device=g.device)
            b.wire = (send, torch.empty_like(send),
                      torch.empty(chunk, dtype=torch.bfloat16, device=g.device),
                      torch.empty_like(send))
        send, recv, own, out = b.wire
        send[:n].copy_(g)
        b.work = ("a2a", dist.all_to_all_single(recv, send, group=self.group, async_op=True))

    def _finish_bf16(self, b: _Bucket):
        """bf16 transport, second half: wait the all-to-all, sum the owned chunk in fp32 in
        rank order, launch the all-gather of the sums (waited by the caller)."""
        _, recv, own, out = b.wire
        chunk = own.numel()
        b.work[1].wait()
        own.copy_(recv.view(self.world, chunk).float().sum(0))
        b.work = ("bf16", dist.all_gather_into_tensor(out, own, group=self.group,
                                                      async_op=True))

    def _codec_segments(self, b: _Bucket) -> List[Tuple[int, int]]:
        if self.codec_scale == "tensor":
            return [(s - b.start, e - b.start) for s, e in (self.flat.span(p) for p in b.params)]
        return [(0, b.end - b.start)]

    def finish(self):
        """Complete all reductions (launch stragglers); compute stream waits, host does not."""
        if self.world == 1:
            return
        if self._calib is not None and self._calib["end"] is None:
            self._calib["end"] = self._now()          # backward's end (before the stragglers)
        if self.proxy:
            # backward's end on the compute stream (proxy_times: bucket end vs backward end)
            if getattr(self, "_bwd_end", None) is None:
                self._bwd_end = torch.cuda.Event(enable_timing=True)
            self._bwd_end.record(torch.cuda.current_stream(self.flat.grad_buf.device))
        if self.codec != "none" and self.codec_scale == "global":
            self._finish_global_codec()
            self._sync = False
            return
        for b in self.buckets:
            if not b.launched:
                self._launch(b)
        if self.codec == "powersgd":
            self._finish_powersgd()
            self._sync = False
            return
        for b in self.buckets:                      # bf16 wire: all-gathers in bucket order
            if isinstance(b.work, tuple) and b.work[0] == "a2a":
                self._finish_bf16(b)
        for b in self.buckets:
            if b.work is None:
                continue
            if isinstance(b.work, tuple) and b.work[0] == "proxy":
                torch.cuda.current_stream(self.flat.grad_buf.device).wait_event(b.work[1])
            elif isinstance(b.work, tuple) and b.work[0] == "bf16":
                b.work[1].wait()
                g = self._seg(b)
                g.copy_(b.wire[3][:g.numel()])
            elif isinstance(b.work, tuple):
                for w in b.work:
                    w.wait()
                self._decode_bucket(b)
            else:
                b.work.wait()
            b.work = None
        self._sync = False                          # disarmed until the next window's last micro-batch

    def _decode_bucket(self, b: _Bucket):
        from ..ops import codec_ops
        g = self._seg(b)
        weights = (C.reference_weights(self.world) if self.reduce == "reference"
                   else [self.weight] * self.world)
        if self.codec == "topk":
            idx, val = ([t.to(g.device) for t in ts] for ts in b.gathered)
            codec_ops.topk_decode_sum(g, idx, val, weights)
        else:
            codec_ops.decode_sum_segments(g, b.gathered[0], b.gathered[1],
                                          self._codec_segments(b), self.codec, weights)
        b.gathered = b.payload = b.scales = None

    def _finish_global_codec(self):
        """Reference-parity mode: one absmax over the WHOLE gradient (ref.py:328-340)."""
        from ..ops import codec_ops
        g = self.flat.grad_buf
        segs = [(0, g.numel())]
        payload, scales = codec_ops.encode_segments(g, segs, self.codec)
        qs = [torch.empty_like(payload) for _ in range(self.world)]
        ss = [torch.empty_like(scales) for _ in range(self.world)]
        dist.all_gather(qs, payload, group=self.group)
        dist.all_gather(ss, scales, group=self.group)
        weights = (C.reference_weights(self.world) if self.reduce == "reference"
                   else [self.weight] * self.world)
        codec_ops.decode_sum_segments(g, qs, ss, segs, self.codec, weights)

    def remove_hooks(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []
