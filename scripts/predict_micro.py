#!/usr/bin/env python
"""Interleaved same-process A/B of the whole-scene prediction head (docs/PERF.md convention).

A: ``head_predict_accum`` — head, softmax and weighted accumulation in one kernel, from the
   last decoder block's pre-BatchNorm output.
B: the unfused composition: ``head_logits`` (fp32 NCHW logits in HBM), ``torch.softmax``,
   the blend weights, one slice-add per window.

Kernel level: 16 disjoint windows of 512^2, C = 32, K = 6.  Scene level: ``ScenePredictor``
on a synthetic 2560 x 2048 scene (depth 5, width / 2, tile 512, overlap 128), fused against
``fused=False``.  Prints one JSON line per level.

``--tta flip|d4`` measures test-time augmentation instead (S = 4 / 8 symmetry codes):

A: the fused kernels with ``codes`` — ``window_gather`` cuts the S views of a window,
   ``head_predict_accum`` un-maps and sums them with one read-modify-write per pixel.
B: the composition without them: the ``codes``-free ops around ``torch.flip`` / ``transpose``
   copies, one accumulate launch per code (blend weights scaled by ``1 / sqrt(S)``, so the
   accumulator is the same).

Both are also reported against S x the single-view (``codes``-free) time, and ``window_gather``
is timed per code on both mappings of the transposing codes: ``lds`` (knob WINDOW_LDS_T = 1)
and ``direct`` (0).  There is one kernel per op — a call without ``codes`` is the list ``[0]`` —
so ``single_view`` and ``plain_16`` time the kernels of code 0 (``plain_16`` and
``code0_direct`` are the same launch, reached without and with a codes tensor)."""
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


def to_view(x, code):
    """[B, T, T, C] window frame -> network side under symmetry ``code`` (flip / transpose copies)."""
    if code & 2:
        x = x.flip(1)
    if code & 1:
        x = x.flip(2)
    if code & 4:
        x = x.transpose(1, 2)
    return x.contiguous()


def to_frame(x, code):
    """The inverse of ``to_view``."""
    if code & 4:
        x = x.transpose(1, 2)
    if code & 2:
        x = x.flip(1)
    if code & 1:
        x = x.flip(2)
    return x.contiguous()


def interleaved(sides, iters, rounds):
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            times[k].append(timed(fn, iters))
    return {k: round(statistics.median(v), 1) for k, v in times.items()}, \
        {k: [round(t, 1) for t in v] for k, v in times.items()}


def kernel_level_tta(a):
    from ddlpc.infer import TTA_CODES, acc_channels, blend_weights
    from ddlpc.ops import _ext
    F = _ext.ops()
    dev = "cuda"
    code_list = list(TTA_CODES[a.tta])
    S = len(code_list)
    B, T, C, K = max(1, 16 // S), a.tile, 32, 6
    H = W = 4 * 2 * T
    torch.manual_seed(0)
    codes = torch.tensor(code_list, dtype=torch.int32, device=dev)
    y = torch.randn(B * S, T, T, C, device=dev).bfloat16()              # window-major views
    bn4 = torch.stack([torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5,
                       torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1]).contiguous()
    wh = torch.randn(K, C, device=dev) * 0.3
    bh = torch.randn(K, device=dev) * 0.1
    win = blend_weights(T, T // 4, "cosine").to(dev)
    win_s = (win / S ** 0.5).contiguous()
    host = [(2 * T * i - T // 8, 2 * T * j - T // 8) for i in range(4) for j in range(4)][:B]
    origins = torch.tensor(host, dtype=torch.int32, device=dev)
    acc_a = torch.zeros(H, W, acc_channels(K), device=dev)
    acc_b = torch.zeros_like(acc_a)
    acc_1 = torch.zeros_like(acc_a)
    yb = y.reshape(B, S, T, T, C).transpose(0, 1).contiguous()          # B's layout: code-major
    y1 = yb[0]

    def fused():
        F.head_predict_accum(y, wh, bh, origins, win, acc_a, bn4, codes)

    def composed():
        for j, c in enumerate(code_list):
            F.head_predict_accum(to_frame(yb[j], c), wh, bh, origins, win_s, acc_b, bn4)

    def single():
        F.head_predict_accum(y1, wh, bh, origins, win, acc_1, bn4)

    fused(), composed()
    err = float((acc_a - acc_b).norm() / acc_b.norm())
    torch.cuda.synchronize()
    med, rounds = interleaved({"fused": fused, "composed": composed, "single_view": single},
                              a.iters, a.rounds)
    print(json.dumps({"level": "kernel", "tta": a.tta, "windows": B, "views": S, "tile": T, "C": C, "K": K,
                      "fused_us": med["fused"], "composed_us": med["composed"],
                      "single_view_us": med["single_view"], "rounds": rounds,
                      "composed_over_fused": round(med["composed"] / med["fused"], 2),
                      "fused_over_S_single": round(med["fused"] / (S * med["single_view"]), 3),
                      "composed_over_S_single": round(med["composed"] / (S * med["single_view"]), 3),
                      "acc_rel_err": err}), flush=True)

    # window_gather: the S views of B windows, per code and for the whole list, on both mappings
    scene = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    one = {c: torch.tensor([c], dtype=torch.int32, device=dev) for c in code_list}
    o16 = torch.tensor([(2 * T * i - T // 8, 2 * T * j - T // 8) for i in range(4) for j in range(4)],
                       dtype=torch.int32, device=dev)
    F.set_knob("WINDOW_LDS_T", 1)
    ref = F.window_gather(scene, origins, T, 8, codes)
    F.set_knob("WINDOW_LDS_T", 0)
    same = bool(torch.equal(F.window_gather(scene, origins, T, 8, codes), ref))
    plain = F.window_gather(scene, origins, T, 8)
    same_b = bool(torch.equal(torch.stack([to_view(plain, c) for c in code_list], 1).reshape(ref.shape), ref))

    def knobbed(v, fn):
        def run():
            F.set_knob("WINDOW_LDS_T", v)
            fn()
        return run

    sides = {"plain_16": knobbed(1, lambda: F.window_gather(scene, o16, T, 8))}
    for c in code_list:                                                   # 16 windows under one code
        for name, v in (("lds", 1), ("direct", 0)):
            sides[f"code{c}_{name}"] = knobbed(v, lambda c=c: F.window_gather(scene, o16, T, 8, one[c]))
    for name, v in (("lds", 1), ("direct", 0)):
        sides[f"{a.tta}_{name}"] = knobbed(v, lambda: F.window_gather(scene, origins, T, 8, codes))

    def gather_composed():
        w = F.window_gather(scene, origins, T, 8)
        return torch.stack([to_view(w, c) for c in code_list], 1)

    sides[f"{a.tta}_composed"] = gather_composed
    med, rounds = interleaved(sides, a.iters, a.rounds)
    F.set_knob("WINDOW_LDS_T", -(2 ** 63))                               # clear the override
    print(json.dumps({"level": "window_gather", "tta": a.tta, "inputs": 16, "tile": T,
                      "lds_equals_direct": same, "equals_flip_transpose": same_b, "us": med,
                      "rounds": rounds}), flush=True)


def scene_level_tta(a):
    from ddlpc import ScenePredictor, UNet
    from ddlpc.data.datasets import engine_input
    from ddlpc.infer import acc_channels
    dev = "cuda"
    torch.manual_seed(0)
    model = UNet(out_classes=6, depth=5, width_divisor=2).to(dev).to_hip()
    scene = torch.randint(0, 256, (a.scene_h, a.scene_w, 3), dtype=torch.uint8, device=dev)
    sp = ScenePredictor(model, a.tile, a.tile // 4, "cosine", a.window_batch, tta=a.tta)
    plain = ScenePredictor(model, a.tile, a.tile // 4, "cosine", a.window_batch)
    code_list, S = list(sp.codes), len(sp.codes)
    F, T = sp.ops, a.tile
    per = max(1, a.window_batch // S)
    win = sp.win.to(dev)
    win_s = (win / S ** 0.5).contiguous()

    @torch.no_grad()
    def composed():
        # the same passes from the codes-free ops: flip / transpose copies on both sides of the
        # forward (one batch of per * S inputs), one accumulate launch per code
        eng = model._engine
        acc = torch.zeros(a.scene_h, a.scene_w, acc_channels(6), device=dev)
        model.eval()
        for host, origins in sp._plan(a.scene_h, a.scene_w, scene.device):
            for i in range(0, len(host), per):
                o = origins[i:i + per]
                w = F.window_gather(scene, o, T, 8)
                x = torch.cat([to_view(w, c) for c in code_list])       # code-major
                y, s = eng.features(engine_input(x, 3), defer_last=True)
                wh, bh = eng._head_params()
                for j, c in enumerate(code_list):
                    n = int(o.shape[0])
                    F.head_predict_accum(to_frame(y[j * n:(j + 1) * n], c), wh.detach().contiguous(),
                                         bh.detach().contiguous(), o, win_s, acc, s)
        model.train()
        return acc

    acc_a, acc_b = sp.accumulate(scene), composed()                       # warm-up
    plain.accumulate(scene)
    err = float((acc_a - acc_b).norm() / acc_b.norm())
    del acc_a, acc_b
    sides = {"fused": lambda: sp.finalize(sp.accumulate(scene)),
             "composed": lambda: sp.finalize(composed()),
             "single_view": lambda: plain.predict(scene)}
    times = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"level": "scene", "tta": a.tta, "H": a.scene_h, "W": a.scene_w, "tile": T,
                      "windows": sp.windows, "inputs": sp.inputs,
                      "fused_ms": round(med["fused"], 2), "composed_ms": round(med["composed"], 2),
                      "single_view_ms": round(med["single_view"], 2),
                      "rounds": {k: [round(t, 2) for t in v] for k, v in times.items()},
                      "composed_over_fused": round(med["composed"] / med["fused"], 3),
                      "fused_over_S_single": round(med["fused"] / (S * med["single_view"]), 3),
                      "acc_rel_err": err}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scene-h", type=int, default=2560)
    ap.add_argument("--scene-w", type=int, default=2048)
    ap.add_argument("--window-batch", type=int, default=16)
    ap.add_argument("--tta", choices=("none", "flip", "d4"), default="none")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_micro.py measures on the GPU; none found")
    if a.tta != "none":
        kernel_level_tta(a)
        scene_level_tta(a)
        return
    kernel_level(a)
    scene_level(a)


if __name__ == "__main__":
    main()
