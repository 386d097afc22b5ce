#!/usr/bin/env python
"""Time ``crop_gather`` per symmetry code at the bench batch (384 x 256^2) from 2500 x 2000
three-channel scenes, with ``tile_gather`` at the same batch shape as the yardstick (the
same bytes of output), interleaved in one process (docs/PERF.md convention).

Every code is timed on both paths of the transposing codes: ``lds`` (knob CROP_LDS_T = 1, the
shipped kernel: bit-4 codes staged through LDS) and ``direct`` (CROP_LDS_T = 0: every code
reads its source pixel straight from HBM; for codes 0..3 the two are the same code path, so
their difference is the run-to-run spread).

``warp_gather`` (random zoom and rotation: 4 bilinear taps and a nearest label per pixel) is
timed at the same batch in the same rounds: ``warp_unit`` with the identity matrix on the rows
``crop_params`` drew (it must write ``crop_gather``'s bits: the cost of the resampling
arithmetic alone), ``warp_z0.5-2_r30`` on rows ``warp_params`` draws from the tables of
``--zoom-min 0.5 --zoom-max 2 --rotate-deg 30``, and ``warp_z0.5_r45`` with every row at zoom
0.5 and 45 degrees (the widest source footprint of that range).  Prints one JSON line per
entry, a markdown table, and the ``warp_gather / crop_gather`` ratios against ``coded4_lds``."""
import argparse
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=384)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--scene-h", type=int, default=2500)
    ap.add_argument("--scene-w", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--jitter", type=float, default=0.1, help="gain / bias jitter of the timed calls")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("crop_micro.py measures on the GPU; none found")
    from ddlpc.data.scenes import ONE, crop_cum, rotation_table, zoom_steps
    from ddlpc.ops import _ext
    F = _ext.ops()
    dev = "cuda"
    B, T, n, H, W = a.batch, a.tile, a.scenes, a.scene_h, a.scene_w
    g = torch.Generator(device=dev).manual_seed(0)
    pixels = torch.randint(0, 256, (n * H * W, 3), dtype=torch.uint8, device=dev, generator=g)
    labels = torch.randint(0, 6, (n * H * W,), dtype=torch.uint8, device=dev, generator=g)
    table = torch.tensor([(k * H * W, H, W) for k in range(n)], dtype=torch.int64)
    cum = torch.from_numpy(crop_cum(table.numpy(), T)).to(dev)
    table = table.to(dev)
    idx = torch.arange(B, dtype=torch.int64, device=dev)
    params, color = F.crop_params(idx, cum, table, 0, T, 2, a.jitter, a.jitter)
    if not a.jitter:
        color = None
    # the yardstick: a tile stack of the scenes' byte count, the same batch shape
    nt = max(B, (n * H * W) // (T * T))
    tiles = pixels[:nt * T * T].reshape(nt, T, T, 3)
    tlab = labels[:nt * T * T].reshape(nt, T, T)
    tidx = torch.randint(0, nt, (B,), device=dev, generator=g)

    entries = {"tile_gather": (None, lambda: F.tile_gather(tiles, tlab, tidx, 8))}
    for code in list(range(8)) + ["d4"]:
        p = params.clone()
        if code != "d4":
            p[:, 3] = code
        for path, knob in (("lds", 1), ("direct", 0)):
            entries[f"code{code}_{path}"] = (knob, lambda p=p: F.crop_gather(pixels, labels, table, p, color, T, 8))
    # warp_gather: the identity on crop_params' rows, rows drawn from the zoom / rotation
    # tables, and the widest footprint (zoom 0.5 at 45 degrees) for every row
    pl = params.long()
    unit = torch.stack([pl[:, 0], (2 * pl[:, 1] + T - 1) * 32768, (2 * pl[:, 2] + T - 1) * 32768, pl[:, 3],
                        torch.full_like(pl[:, 0], ONE), torch.zeros_like(pl[:, 0])], 1).contiguous()
    steps = torch.from_numpy(zoom_steps(0.5, 2.0)).to(dev)
    rot = torch.from_numpy(rotation_table(30.0)).to(dev)
    drawn, _ = F.warp_params(idx, cum, table, steps, rot, 0, T, 2, a.jitter, a.jitter)
    wide, _ = F.warp_params(idx, cum, table, torch.full_like(steps, 2 * ONE),
                            torch.from_numpy(rotation_table(0.0)).to(dev), 0, T, 2, a.jitter, a.jitter)
    wide[:, 4] = wide[:, 5] = int(round(2 * ONE * 0.5 ** 0.5))
    warps = {"warp_unit": unit, "warp_z0.5-2_r30": drawn, "warp_z0.5_r45": wide}
    for name, w in warps.items():
        entries[name] = (None, lambda w=w: F.warp_gather(pixels, labels, table, w, color, T, 8))
    times = {k: [] for k in entries}

    def run(name, iters):
        knob, fn = entries[name]
        if knob is not None:
            F.set_knob("CROP_LDS_T", knob)
        return timed(fn, iters)

    for name in entries:
        run(name, 3)                                     # warm-up
    for code in list(range(8)) + ["d4"]:                 # the two paths write the same bits
        outs = []
        for path in ("lds", "direct"):
            knob, fn = entries[f"code{code}_{path}"]
            F.set_knob("CROP_LDS_T", knob)
            outs.append(fn())
        if not (torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])):
            raise SystemExit(f"code {code}: the lds and the direct path differ")
    F.set_knob("CROP_LDS_T", 1)
    outs = [entries["coded4_lds"][1](), entries["warp_unit"][1]()]
    if not (torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])):
        raise SystemExit("warp_gather with the identity matrix differs from crop_gather")
    del outs
    for _ in range(a.rounds):
        for name in entries:
            times[name].append(run(name, a.iters))
    F.set_knob("CROP_LDS_T", -(2 ** 63))                 # clear the override
    out_bytes = B * T * T * (16 + 8)
    res = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = med
        print(json.dumps({"entry": name, "batch": B, "tile": T, "us": round(med, 1),
                          "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                          "out_gb_s": round(out_bytes / med * 1e-3, 1)}), flush=True)
    print(f"\n| entry ({B} x {T}^2) | us (median of {a.rounds}) | min .. max | x tile_gather |")
    print("|---|---|---|---|")
    for name, ts in times.items():
        print(f"| {name} | {res[name]:.1f} | {min(ts):.1f} .. {max(ts):.1f} | "
              f"{res[name] / res['tile_gather']:.2f} |")
    print()
    for name in warps:
        print(json.dumps({"ratio": f"{name} / coded4_lds", "value": round(res[name] / res["coded4_lds"], 3)}),
              flush=True)


if __name__ == "__main__":
    main()
