#!/usr/bin/env python
"""Time the optimizer step on the default model's flat buffer (about 8.7 M fp32 parameters):
``adam_step_dev`` against ``adam_step_sched`` with clipping off and on (coupled and decoupled
decay), interleaved in one process.  Each variant is timed with device events over ``--inner``
back-to-back calls, ``--repeats`` times round-robin after a warm-up; the median per call is
reported with the bytes each variant must move (7 streams of n floats for Adam, one more read of
g for the norm) and the HBM rate that implies.  Prints one JSON line (docs/PERF.md records it).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=0, help="elements (0: the default U-Net's parameter count)")
    a = ap.parse_args()
    from ddlpc.models import UNet
    from ddlpc.ops import _ext
    from ddlpc.ops.adam import grad_sqnorm_blocks
    o = _ext.ops()
    n = a.n or sum(p.numel() for p in UNet(out_classes=6).parameters())
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=g).to(dev)
    grad = (torch.randn(n, generator=g) * 1e-2).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    scal3, scal8 = torch.zeros(3, device=dev), torch.zeros(8, device=dev)
    partial = torch.zeros(grad_sqnorm_blocks(n), dtype=torch.float64, device=dev)
    hp = (1e-3, 0.9, 0.999, 1e-8)

    def sched(wd, decoupled, max_norm):
        return lambda: o.adam_step_sched(p, grad, m, v, scal8, partial, *hp, wd, decoupled, max_norm, 2, 100,
                                         100000, 1e-5, 0.9)
    variants = {
        "adam_step_dev": (lambda: o.adam_step_dev(p, grad, m, v, scal3, *hp, 0.0), 7),
        "adam_step_sched": (sched(0.0, False, 0.0), 7),
        "adam_step_sched clip": (sched(0.0, False, 1.0), 8),
        "adam_step_sched clip adamw": (sched(0.01, True, 1.0), 8),
    }
    times = {k: [] for k in variants}
    for r in range(a.warmup + a.repeats):
        for name, (fn, _) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    out = {"n": n, "repeats": a.repeats, "inner": a.inner, "device": torch.cuda.get_device_name(0)}
    for name, (_, streams) in variants.items():
        t = sorted(times[name])
        med = statistics.median(t)
        out[name] = {"median_us": round(med, 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2),
                     "streams": streams, "gb_per_s": round(streams * 4 * n / med / 1e3, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
