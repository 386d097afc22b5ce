#!/usr/bin/env python
"""Micro-benchmark of the label operators (csrc/boundary.hip) next to the pass they precede.

The flagship validation batch (384 x 256^2 int64 labels, a coarse random class grid up-sampled as
the synthetic tiles are): ``label_erode`` at r = 3 (the ISPRS disc) and r = 16, ``label_dist2``, and
``head_eval`` (C = 32, deferred BN) on the same batch, alternated in one process; then one 2500 x
2000 uint8 scene: ``label_erode`` at r = 3 and ``scene_finalize`` with labels.  One line each with
median, min and max over ``--rounds`` of ``--iters`` launches between two device events."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, iters):
    """seconds per call over ``iters`` calls between two device events (after one warm call)"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def labels_like_tiles(shape, K, grid, dev, g, dtype):
    coarse = torch.randint(0, K, shape[:-2] + (grid, grid), generator=g, device=dev).float()
    lab = torch.nn.functional.interpolate(coarse.reshape(-1, 1, grid, grid), size=shape[-2:], mode="nearest")
    return lab.reshape(shape).to(dtype).contiguous()


def run(fns, rounds, iters):
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn, iters))
    for k, t in ts.items():
        print(f"{k:28s} median {statistics.median(t) * 1e6:9.1f} us  min {min(t) * 1e6:9.1f}  "
              f"max {max(t) * 1e6:9.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    from ddlpc.ops import _ext
    F, dev, K, C, H = _ext.ops(), "cuda", 6, 32, 256
    g = torch.Generator(device=dev).manual_seed(0)
    lab = labels_like_tiles((a.batch, H, H), K, 8, dev, g, torch.int64)
    y = torch.randn(a.batch, H, H, C, device=dev, generator=g).bfloat16()
    bn4 = torch.stack([torch.randn(C, device=dev, generator=g) * 0.1, torch.rand(C, device=dev, generator=g) + 0.5,
                       torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g) * 0.1])
    wh, bh = torch.randn(K, C, device=dev, generator=g) * 0.3, torch.randn(K, device=dev, generator=g) * 0.1
    sums = torch.zeros(3, dtype=torch.float64, device=dev)
    cm = torch.zeros(K, K, dtype=torch.int64, device=dev)
    band = float((F.label_erode(lab, K, -100, 3, -100) != lab).float().mean())
    print(f"batch {a.batch} x {H}^2 int64, {band:.1%} of the pixels in the r = 3 band", flush=True)
    run({"label_erode r=3 int64": lambda: F.label_erode(lab, K, -100, 3, -100),
         "label_erode r=16 int64": lambda: F.label_erode(lab, K, -100, 16, -100),
         "label_dist2 int64": lambda: F.label_dist2(lab, K, -100),
         "head_eval C=32": lambda: F.head_eval(y, wh, bh, lab, -100, sums, cm, bn4)}, a.rounds, a.iters)
    del y, lab
    scene = labels_like_tiles((2500, 2000), K, 40, dev, g, torch.uint8)
    acc = torch.rand(2500, 2000, 8, device=dev, generator=g)
    print("scene 2500 x 2000 uint8", flush=True)
    run({"label_erode r=3 uint8": lambda: F.label_erode(scene, K, -100, 3, 255),
         "scene_finalize + labels": lambda: F.scene_finalize(acc, K, scene, -100)}, a.rounds, a.iters)


if __name__ == "__main__":
    main()
