#!/usr/bin/env python
"""Time the gradient codecs on one 8 MB bucket (2 Mi fp32 gradients), world 2, in one process:

* ``topk_encode`` + ``topk_decode_sum`` at ratios 0.001 / 0.01 / 0.1 (csrc/topk.hip), encode
  and decode also on their own; the encode's residual is re-filled outside the timed window
  so every repeat selects from the same data;
* next to them the int8 codec's ``codec_absmax`` + ``codec_encode`` + ``codec_decode_sum``
  (csrc/misc.hip) on the same bucket;
* the low-rank codec on the flagship model's whole gradient buffer (the default ``TrainConfig``
  model, ``--mb`` buckets, ``--rank``): the five ``psgd_*`` kernels of every bucket, no
  collective (csrc/powersgd.hip), each of the five also on its own; next to it, on the same
  buffer and buckets, ``topk_encode`` + ``topk_decode_sum`` at ratio 0.01 and a plain device copy.

Each variant is timed with device events over ``--inner`` back-to-back calls, ``--repeats``
times round-robin after a warm-up; the median, min and max per call are reported, with the
wire bytes of one rank's payload (arithmetic).  ``--trace`` runs a few untimed calls of every
variant only, for a kernel trace taken by a profiler around this script (the per-kernel split
of the encode: select passes / count / compact).  Prints one JSON line (docs/PERF.md).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATIOS = (0.001, 0.01, 0.1)


def powersgd_variants(variants, o, dev, mb, rank, gen):
    """The flagship model's gradient buffer in the reducer's buckets: the five psgd_* kernels of
    every bucket (together and one by one), top-k at 0.01 and a device copy on the same buffer."""
    from ddlpc.config import TrainConfig
    from ddlpc.models.unet import UNet
    from ddlpc.parallel import codec as C
    from ddlpc.parallel.flat import FlatParams
    from ddlpc.parallel.reducer import GradBucketReducer
    flat = FlatParams([p for p in UNet.from_config(TrainConfig().model).to(dev).parameters() if p.requires_grad])
    red = GradBucketReducer(flat, bucket_mb=mb, grad_codec="powersgd", powersgd_rank=rank)
    g = flat.grad_buf
    g.copy_((torch.randn(g.numel(), generator=gen) * 1e-3).to(dev))
    sts = [(b, red._psgd_buffers(b)) for b in red.buckets]
    e, out, w = red.residual, torch.empty_like(g), torch.full((2,), 0.5, device=dev)
    steps = {
        "project": lambda b, s: o.psgd_project(g[b.start:b.end], e[b.start:b.end], s.q_prev, s.wire_p, s.low, s.raw, rank, 0.5),
        "orthonormalize": lambda b, s: o.psgd_orthonormalize(s.wire_p, s.low, rank),
        "backproject": lambda b, s: o.psgd_backproject(e[b.start:b.end], s.wire_p, s.q_loc, s.wire_q, s.low, rank, 0.5),
        "residual": lambda b, s: o.psgd_residual(e[b.start:b.end], s.wire_p, s.q_loc, s.low, rank),
        "decode": lambda b, s: o.psgd_decode(g[b.start:b.end], s.wire_p, s.wire_q, s.low, s.raw, rank),
    }

    def exchange(names=tuple(steps)):
        for name in names:
            for b, s in sts:
                steps[name](b, s)

    def topk():
        for b, _ in sts:
            k = C.topk_count(b.end - b.start, 0.01)
            i, v = o.topk_encode(g[b.start:b.end], e[b.start:b.end], k)
            o.topk_decode_sum(out[b.start:b.end], torch.stack([i, i]), torch.stack([v, v]), w)
    exchange()                                      # (the tables' check on the host)
    variants[f"model powersgd r{rank} exchange"] = exchange
    for name in steps:
        variants[f"model powersgd r{rank} {name}"] = lambda name=name: exchange((name,))
    variants["model topk 0.01 encode+decode_sum"] = topk
    variants["model device copy"] = lambda: out.copy_(g)
    return {"floats": g.numel(), "buckets": len(sts), **{k: v for k, v in red.stats.items() if "powersgd" in k}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mb", type=float, default=8.0, help="bucket size (fp32 gradient MB)")
    ap.add_argument("--rank", type=int, default=4, help="powersgd rank")
    ap.add_argument("--trace", action="store_true", help="a few calls of each variant, no timing")
    a = ap.parse_args()
    from ddlpc.ops import _ext
    from ddlpc.parallel import codec as C
    o = _ext.ops()
    n = int(a.mb * (1 << 20)) // 4
    world = 2
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    g = (torch.randn(n, generator=gen) * 1e-3).to(dev)
    e0 = (torch.randn(n, generator=gen) * 1e-3).to(dev)          # a non-trivial residual
    e = e0.clone()
    out = torch.empty_like(g)
    w = torch.full((world,), 1.0 / world, device=dev)
    seg = torch.tensor([0, n], dtype=torch.int64, device=dev)

    variants, wire = {}, {"fp32": 4 * n, "fp16_absmax": 2 * n + 4, "int8_absmax": n + 4}
    for ratio in RATIOS:
        k = C.topk_count(n, ratio)
        wire[f"topk {ratio}"] = 8 * k
        idx, val = o.topk_encode(g, e0.clone(), k)
        idx2, val2 = torch.stack([idx, idx]), torch.stack([val, val])

        def enc(k=k):
            o.topk_encode(g, e, k)

        def dec(idx2=idx2, val2=val2):
            o.topk_decode_sum(out, idx2, val2, w)

        def both(k=k):
            i, v = o.topk_encode(g, e, k)
            o.topk_decode_sum(out, torch.stack([i, i]), torch.stack([v, v]), w)
        variants[f"topk {ratio} encode"] = enc
        variants[f"topk {ratio} decode_sum"] = dec
        variants[f"topk {ratio} encode+decode_sum"] = both
    sc = o.codec_absmax(g, seg)
    q2, s2 = torch.stack([o.codec_encode(g, seg, sc, 1)] * 2), torch.stack([sc, sc])

    def int8_enc():
        s = o.codec_absmax(g, seg)
        o.codec_encode(g, seg, s, 1)

    def int8_dec():
        o.codec_decode_sum(out, q2, s2, w, seg, 1)

    def int8_both():
        s = o.codec_absmax(g, seg)
        q = o.codec_encode(g, seg, s, 1)
        o.codec_decode_sum(out, torch.stack([q, q]), torch.stack([s, s]), w, seg, 1)
    variants["int8 absmax+encode"] = int8_enc
    variants["int8 decode_sum"] = int8_dec
    variants["int8 absmax+encode+decode_sum"] = int8_both
    model = powersgd_variants(variants, o, dev, a.mb, a.rank, gen)

    if a.trace:
        for fn in variants.values():
            for _ in range(3):
                e.copy_(e0)
                fn()
        torch.cuda.synchronize()
        return
    times = {name: [] for name in variants}
    for r in range(a.warmup + a.repeats):
        for name, fn in variants.items():
            e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e.copy_(e0)
            e0_.record()
            for _ in range(a.inner):
                fn()
            e1_.record()
            e1_.synchronize()
            if r >= a.warmup:
                times[name].append(e0_.elapsed_time(e1_) * 1e3 / a.inner)
    res = {"n": n, "world": world, "repeats": a.repeats, "inner": a.inner,
           "device": torch.cuda.get_device_name(0), "wire_bytes_per_rank": wire, "model": model}
    for name, t in times.items():
        t = sorted(t)
        res[name] = {"median_us": round(statistics.median(t), 2), "min_us": round(t[0], 2),
                     "max_us": round(t[-1], 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
