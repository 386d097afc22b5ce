#!/usr/bin/env python
"""Micro-benchmark of the fused head kernels at the flagship shape (256^2, 32 channels, 6 classes,
deferred BN).

``--mode train`` (default, batch 128): the training forward + statistics pass and the recompute +
BN-backward apply pass.  Run under rocprofv3 --pmc for counters.  ``--class-weights`` times the
class-weighted instantiations of the same kernels.

``--mode eval`` (batch 384, the bench shape): the evaluation head ``head_eval`` against
``head_logits`` followed by the stock composition ``Trainer.validate`` ran before it
(cross_entropy, argmax, bincount), alternated in one process at the same pixel count: one line per
width (C = 32 and the channel-split C = 64) with median, min and max over ``--rounds`` and the
achieved bytes/s of ``head_eval`` (2 C + 8 bytes per pixel).  A third line times ``head_eval`` on
a one-class region (every pixel bumps the same counter).

``--mode validate``: a full ``Trainer.validate()`` pass over ``--samples`` synthetic tiles with
``fused_eval`` on and off, alternated."""
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


def line(name, ts, nbytes=None):
    med = statistics.median(ts)
    rate = f"  {nbytes / med / 1e12:5.2f} TB/s" if nbytes else ""
    print(f"{name:24s} median {med * 1e6:9.1f} us  min {min(ts) * 1e6:9.1f}  max {max(ts) * 1e6:9.1f}{rate}", flush=True)
    return med


def train_mode(a, F, dev):
    N, H, C, K = a.batch or 128, 256, 32, 6
    y = torch.randn(N, H, H, C, device=dev).bfloat16()
    bn4 = torch.stack([torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5,
                       torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1]).contiguous()
    wh = torch.randn(K, C, device=dev) * 0.3
    bh = torch.randn(K, device=dev) * 0.1
    lab = torch.randint(0, K, (N, H, H), device=dev)
    gamma = torch.rand(C, device=dev) + 0.5
    # (class_weight is passed only when asked for: the script also runs on builds without it)
    kw = {"class_weight": torch.tensor([0.3, 0.5, 3.0, 0.7, 1.9, 1.0], device=dev)} if a.class_weights else {}
    o, wrows, brows = F.head_ce_fwd_stats(y, wh, bh, lab, -100, bn4, **kw)
    scale = torch.ones(1, device=dev) / o[2:3]
    fns = {"fwd_stats": lambda: F.head_ce_fwd_stats(y, wh, bh, lab, -100, bn4, **kw),
           "bn_apply": lambda: F.head_ce_bn_bwd(y, wh, bh, lab, o, None, -100, bn4, brows, gamma,
                                                None, None, scale, **kw)}
    tag = "+w" if a.class_weights else ""
    for name, fn in fns.items():
        print(f"{name + tag:10s} {timed(fn, a.iters) * 1e6:8.1f} us", flush=True)


def eval_mode(a, F, dev):
    N, H, K = a.batch or 384, 256, 6
    for C in (32, 64):
        g = torch.Generator(device=dev).manual_seed(C)
        y = torch.randn(N, H, H, C, device=dev, generator=g).bfloat16()
        bn4 = torch.stack([torch.randn(C, device=dev, generator=g) * 0.1, torch.rand(C, device=dev, generator=g) + 0.5,
                           torch.rand(C, device=dev, generator=g) + 0.5,
                           torch.randn(C, device=dev, generator=g) * 0.1]).contiguous()
        wh = torch.randn(K, C, device=dev, generator=g) * 0.3
        bh = torch.randn(K, device=dev, generator=g) * 0.1
        lab = torch.randint(0, K, (N, H, H), device=dev, generator=g)
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        cm = torch.zeros(K, K, dtype=torch.int64, device=dev)
        acc, cmf = torch.zeros(3, dtype=torch.float64, device=dev), torch.zeros(K * K, dtype=torch.float64, device=dev)

        def fused(lab=lab, bh=bh):
            F.head_eval(y, wh, bh, lab, -100, sums, cm, bn4)

        def composed():       # the loop body of Trainer.validate on the logits path
            logits = F.head_logits(y, wh, bh, bn4).float()
            loss = torch.nn.functional.cross_entropy(logits, lab, reduction="sum")
            pred = logits.argmax(1)
            acc.add_(torch.stack([loss.double(), (pred == lab).sum().double(),
                                  torch.tensor(float(lab.numel()), device=dev, dtype=torch.float64)]))
            cmf.add_(torch.bincount((lab * K + pred).reshape(-1), minlength=K * K).double())

        fused()
        composed()
        torch.cuda.synchronize()
        # (the two paths round their fp32 logits differently: near-ties may fall either way)
        moved = int((cm.double().reshape(-1) - cmf).abs().sum()) // 2
        rel = abs(float(sums[0]) - float(acc[0])) / abs(float(acc[0]))
        print(f"C={C}: {moved} of {lab.numel()} pixels predicted differently, loss sums differ by {rel:.2e} (relative)",
              flush=True)
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(timed(fused, a.iters))
            tb.append(timed(composed, a.iters))
        nbytes = N * H * H * (2 * C + 8)
        ma = line(f"head_eval C={C}", ta, nbytes)
        mb = line(f"logits + torch C={C}", tb)
        print(f"  -> {mb / ma:.2f}x", flush=True)
        if C == 32:           # a one-class region: every counted pixel bumps counter [0][0]
            b1 = bh.clone()
            b1[0] += 1e4
            l1 = torch.zeros_like(lab)
            line("head_eval C=32 one class", [timed(lambda: fused(l1, b1), a.iters) for _ in range(a.rounds)], nbytes)
        del y, lab
        torch.cuda.empty_cache()


def validate_mode(a, dev):
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.train.trainer import Trainer
    trs = {}
    for fused in (True, False):
        cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=256, batch_per_gpu=a.batch or 384,
                          num_samples=a.samples + 1, test_holdout=a.samples, impl="hip", log_dir=None, log_every=0,
                          fused_eval=fused).validate()
        trs[fused] = Trainer(cfg, device=dev)
    res = {f: tr.validate() for f, tr in trs.items()}       # warm, and the two paths' results
    print({f: (r["val_loss"], r["val_pixel_acc"], r["val_miou"]) for f, r in res.items()}, flush=True)
    ts = {True: [], False: []}
    for _ in range(a.rounds):
        for f, tr in trs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.validate()                                    # (ends in .tolist(): the device has finished)
            e1.record()
            e1.synchronize()
            ts[f].append(e0.elapsed_time(e1) * 1e-3)
    ma = line(f"validate fused   n={a.samples}", ts[True])
    mb = line(f"validate logits  n={a.samples}", ts[False])
    print(f"  -> {mb / ma:.3f}x", flush=True)
    for tr in trs.values():
        tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="train", choices=["train", "eval", "validate"])
    ap.add_argument("--batch", type=int, default=None, help="default: 128 (train), 384 (eval, validate)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7, help="eval / validate: alternated timing rounds")
    ap.add_argument("--samples", type=int, default=768, help="validate: tiles in the held-out split")
    ap.add_argument("--class-weights", action="store_true", help="train: pass class_weight (6 values)")
    a = ap.parse_args()
    from ddlpc.ops import _ext
    F = _ext.ops()
    dev = "cuda"
    if a.mode == "train":
        train_mode(a, F, dev)
    elif a.mode == "eval":
        eval_mode(a, F, dev)
    else:
        validate_mode(a, dev)


if __name__ == "__main__":
    main()
