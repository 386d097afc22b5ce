#!/usr/bin/env python
"""Interleaved same-process A/B of the whole-scene prediction head (docs/PERF.md convention).

A: ``head_predict_accum`` — head, softmax and weighted accumulation in one kernel, from the
   last decoder block's pre-BatchNorm output.
B: the unfused composition: ``head_logits`` (fp32 NCHW logits in HBM), ``torch.softmax``,
   the blend weights, one slice-add per window.

Kernel level: 16 disjoint windows of 512^2, C = 32, K = 6.  Scene level: ``ScenePredictor``
on a synthetic 2560 x 2048 scene (depth 5, width / 2, tile 512, overlap 128), fused against
``fused=False``.  Prints one JSON line per level."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters            # us


def kernel_level(a):
    from ddlpc.infer import acc_channels, blend_weights
    from ddlpc.ops import _ext
    F = _ext.ops()
    dev = "cuda"
    B, T, C, K = 16, a.tile, 32, 6
    H = W = 4 * 2 * T
    torch.manual_seed(0)
    y = torch.randn(B, T, T, C, device=dev).bfloat16()
    bn4 = torch.stack([torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5,
                       torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1]).contiguous()
    wh = torch.randn(K, C, device=dev) * 0.3
    bh = torch.randn(K, device=dev) * 0.1
    win = blend_weights(T, T // 4, "cosine").to(dev)
    w2 = win[:, None] * win[None, :]
    host = [(2 * T * i - T // 8, 2 * T * j - T // 8) for i in range(4) for j in range(4)]
    origins = torch.tensor(host, dtype=torch.int32, device=dev)
    acc_a = torch.zeros(H, W, acc_channels(K), device=dev)
    acc_b = torch.zeros_like(acc_a)

    def fused():
        F.head_predict_accum(y, wh, bh, origins, win, acc_a, bn4)

    def unfused():
        p = torch.softmax(F.head_logits(y, wh, bh, bn4), dim=1) * w2
        for b, (y0, x0) in enumerate(host):
            ys, xs = max(0, -y0), max(0, -x0)
            dst = acc_b[y0 + ys:y0 + T, x0 + xs:x0 + T]
            dst[..., :K] += p[b, :, ys:, xs:].permute(1, 2, 0)
            dst[..., K] += w2[ys:, xs:]

    fused(), unfused()
    err = float((acc_a - acc_b).norm() / acc_b.norm())
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(timed(fused, a.iters))
        tb.append(timed(unfused, a.iters))
    A, Bm = statistics.median(ta), statistics.median(tb)
    print(json.dumps({"level": "kernel", "windows": B, "tile": T, "C": C, "K": K,
                      "fused_us": round(A, 1), "unfused_us": round(Bm, 1),
                      "fused_us_rounds": [round(t, 1) for t in ta],
                      "unfused_us_rounds": [round(t, 1) for t in tb],
                      "unfused_over_fused": round(Bm / A, 2), "acc_rel_err": err}), flush=True)


def scene_level(a):
    from ddlpc import ScenePredictor, UNet
    dev = "cuda"
    torch.manual_seed(0)
    model = UNet(out_classes=6, depth=5, width_divisor=2).to(dev).to_hip()
    scene = torch.randint(0, 256, (a.scene_h, a.scene_w, 3), dtype=torch.uint8, device=dev)
    sides = {"fused": ScenePredictor(model, a.tile, a.tile // 4, "cosine", a.window_batch),
             "unfused": ScenePredictor(model, a.tile, a.tile // 4, "cosine", a.window_batch, fused=False)}
    accs = {k: sp.accumulate(scene) for k, sp in sides.items()}          # warm-up
    err = float((accs["fused"] - accs["unfused"]).norm() / accs["unfused"].norm())
    del accs
    times = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, sp in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sp.predict(scene)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    A, Bm = statistics.median(times["fused"]), statistics.median(times["unfused"])
    print(json.dumps({"level": "scene", "H": a.scene_h, "W": a.scene_w, "tile": a.tile,
                      "windows": sides["fused"].windows, "fused_ms": round(A, 2),
                      "unfused_ms": round(Bm, 2),
                      "fused_ms_rounds": [round(t, 2) for t in times["fused"]],
                      "unfused_ms_rounds": [round(t, 2) for t in times["unfused"]],
                      "unfused_over_fused": round(Bm / A, 3), "acc_rel_err": err}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scene-h", type=int, default=2560)
    ap.add_argument("--scene-w", type=int, default=2048)
    ap.add_argument("--window-batch", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_micro.py measures on the GPU; none found")
    kernel_level(a)
    scene_level(a)


if __name__ == "__main__":
    main()
