"""Bodies of the whole-scene prediction tests, written once and run on both kernel sets:
``test_predict_cpu.py`` passes ``"cpu"`` (the C++ kernels of ``csrc/cpu_ref.cpp``),
``test_predict_gpu.py`` passes ``"cuda"`` (the gfx950 kernels)."""
import math

import torch

PLAN_CASES = [(70, 52, 32, 16), (70, 52, 32, 8), (33, 95, 32, 0), (20, 20, 32, 16), (5, 7, 16, 8)]
HEAD_CASES = [(32, 6), (16, 3), (64, 11), (8, 16)]
PREDICTOR_SHAPES = [(70, 52, 32, 16), (33, 95, 32, 0), (20, 20, 32, 16)]
MODELS = {"d3_convt": dict(depth=3, width_divisor=2, out_classes=6, up_sample_mode="conv_transpose"),
          "d2_bilinear": dict(depth=2, width_divisor=4, out_classes=3, up_sample_mode="bilinear")}


def ops():
    from ddlpc.ops import _ext
    return _ext.ops()


def rel_err(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def rand_scene(H, W, seed, device, in_ch=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (H, W, in_ch), generator=g, dtype=torch.uint8).to(device)


# ------------------------------------------------------------------ plan (no kernels)
def weight_sum_map(H, W, tile, overlap, blend):
    from ddlpc.infer import blend_weights, plan_windows
    w = blend_weights(tile, overlap, blend)
    w2 = w[:, None] * w[None, :]
    out = torch.zeros(H, W)
    for group in plan_windows(H, W, tile, overlap):
        for y0, x0 in group:
            ys, xs, ye, xe = max(0, -y0), max(0, -x0), min(tile, H - y0), min(tile, W - x0)
            if ye > ys and xe > xs:
                out[y0 + ys:y0 + ye, x0 + xs:x0 + xe] += w2[ys:ye, xs:xe]
    return out


def check_plan(H, W, tile, overlap):
    from ddlpc.infer import blend_weights, plan_windows
    groups = plan_windows(H, W, tile, overlap)
    s, m = tile - overlap, overlap // 2
    assert len(groups) == 4
    assert sum(len(g) for g in groups) == math.ceil(H / s) * math.ceil(W / s)
    cores = torch.zeros(H, W, dtype=torch.int64)
    for colour, group in enumerate(groups):
        assert group == sorted(group)                                   # row-major
        for n, (y0, x0) in enumerate(group):
            i, j = (y0 + m) // s, (x0 + m) // s
            assert (y0 + m) % s == 0 and (x0 + m) % s == 0 and 2 * (i & 1) + (j & 1) == colour
            for y1, x1 in group[:n]:                                    # pairwise disjoint
                assert abs(y1 - y0) >= tile or abs(x1 - x0) >= tile
            cy, cx = y0 + m, x0 + m
            cores[max(cy, 0):min(cy + s, H), max(cx, 0):min(cx + s, W)] += 1
    assert torch.equal(cores, torch.ones_like(cores))                   # cores partition the scene
    for blend in ("core", "cosine"):
        w = blend_weights(tile, overlap, blend)
        assert w.dtype == torch.float32 and w.shape == (tile,)
        if overlap == 0:
            assert torch.equal(w, torch.ones(tile))
        wsum = weight_sum_map(H, W, tile, overlap, blend)
        assert float(wsum.min()) > 0
        if blend == "core":
            assert torch.equal(wsum, torch.ones(H, W))
        else:
            assert float(wsum.min()) >= 0.25
            inner = wsum[m:H - m, m:W - m]
            assert inner.numel() > 0 or min(H, W) <= 2 * m    # (a scene of borders only)
            if inner.numel():
                assert float((inner - 1).abs().max()) < 1e-6


# ------------------------------------------------------------------ window_gather
def check_window_gather(device, H, W, tile, overlap):
    from ddlpc.infer import plan_windows, reflect
    scene = rand_scene(H, W, 1, device)
    origins = [o for g in plan_windows(H, W, tile, overlap) for o in g]
    origins += [(-tile + 1, -tile + 1), (H - 1, W - 1), (-3, W - 2), (H - 2, -5)]   # all four sides
    o = torch.tensor(origins, dtype=torch.int32, device=device)
    got = ops().window_gather(scene, o, tile, 8)
    assert got.dtype == torch.bfloat16 and got.shape == (len(origins), tile, tile, 8)
    ref = torch.zeros(len(origins), tile, tile, 8, device=device)
    for b, (y0, x0) in enumerate(origins):
        iy = torch.tensor([reflect(y0 + t, H) for t in range(tile)], device=device)
        ix = torch.tensor([reflect(x0 + t, W) for t in range(tile)], device=device)
        ref[b, :, :, :3] = scene.index_select(0, iy).index_select(1, ix).float() / 255
    assert torch.equal(got, ref.bfloat16())


# ------------------------------------------------------------------ head_predict_accum
HEAD_ORIGINS = [(-4, -4), (-4, 12), (12, -4), (28, 12)]


def _bn4(C, device):
    g = torch.Generator().manual_seed(11)
    return torch.stack([torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5,
                        torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.3]).to(device).contiguous()


def check_head_predict_accum(device, C, K, blend):
    """-> the measured rel_err of the added part (printed by the callers)."""
    from ddlpc.infer import acc_channels, blend_weights
    F = ops()
    H, W, tile = 40, 27, 16
    KA = acc_channels(K)
    assert KA == {6: 8, 3: 4, 11: 12, 16: 20}[K]
    g = torch.Generator().manual_seed(5)
    B = len(HEAD_ORIGINS)
    a = torch.relu(torch.randn(B, tile, tile, C, generator=g)).bfloat16().to(device)
    wh = (torch.randn(K, C, generator=g) * 0.3).to(device)
    bh = (torch.randn(K, generator=g) * 0.1).to(device)
    fill = torch.randn(H, W, KA, generator=g).to(device)
    win = blend_weights(tile, 8, blend).to(device)
    o = torch.tensor(HEAD_ORIGINS, dtype=torch.int32, device=device)
    acc = fill.clone()
    F.head_predict_accum(a, wh, bh, o, win, acc)
    # fp32 torch on the same bf16 activation
    p = torch.softmax(a.float() @ wh.t() + bh, dim=-1)
    w2 = win[:, None] * win[None, :]
    add = torch.zeros(H, W, KA, device=device)
    for b, (y0, x0) in enumerate(HEAD_ORIGINS):
        ys, xs, ye, xe = max(0, -y0), max(0, -x0), min(tile, H - y0), min(tile, W - x0)
        add[y0 + ys:y0 + ye, x0 + xs:x0 + xe, :K] = p[b, ys:ye, xs:xe] * w2[ys:ye, xs:xe, None]
        add[y0 + ys:y0 + ye, x0 + xs:x0 + xe, K] = w2[ys:ye, xs:xe]
    touched = add[..., K] != 0
    assert 0 < int(touched.sum()) < H * W
    err = rel_err(acc - fill, add)
    print(f"head_predict_accum C={C} K={K} {blend}: rel_err {err:.3e}")
    assert err < 1e-4
    assert torch.equal(acc[..., K + 1:], fill[..., K + 1:])             # channels above K
    assert torch.equal(acc[~touched], fill[~touched])                   # uncovered / zero weight
    # deferred BatchNorm: bit-identical to the call on the materialised activation
    y = torch.randn(B, tile, tile, C, generator=g).bfloat16().to(device)
    bn4 = _bn4(C, device)
    act = F.bn_relu_apply(y, bn4, False)[0]
    acc_d, acc_m = fill.clone(), fill.clone()
    F.head_predict_accum(y, wh, bh, o, win, acc_d, bn4)
    F.head_predict_accum(act, wh, bh, o, win, acc_m)
    assert torch.equal(acc_d, acc_m)
    assert not torch.equal(acc_d, fill)
    return err


def check_head_predict_accum_rejects(device):
    import pytest
    F = ops()
    a = torch.zeros(1, 16, 16, 32, dtype=torch.bfloat16, device=device)
    wh, bh = torch.zeros(6, 32, device=device), torch.zeros(6, device=device)
    o = torch.zeros(1, 2, dtype=torch.int32, device=device)
    win = torch.ones(16, device=device)
    with pytest.raises(RuntimeError):                                   # KA must be 8 for K = 6
        F.head_predict_accum(a, wh, bh, o, win, torch.zeros(20, 20, 7, device=device))
    with pytest.raises(RuntimeError):                                   # int32 origins
        F.head_predict_accum(a, wh, bh, o.long(), win, torch.zeros(20, 20, 8, device=device))
    with pytest.raises(RuntimeError):                                   # unsupported C
        F.head_predict_accum(torch.zeros(1, 16, 16, 24, dtype=torch.bfloat16, device=device),
                             torch.zeros(6, 24, device=device), bh, o, win,
                             torch.zeros(20, 20, 8, device=device))


# ------------------------------------------------------------------ scene_finalize
def check_scene_finalize(device, K):
    from ddlpc.infer import acc_channels
    F = ops()
    H, W = 37, 29
    g = torch.Generator().manual_seed(K)
    acc = torch.rand(H, W, acc_channels(K), generator=g)
    acc[..., K:] = 7.0                                                  # never the arg-max
    for n in range(0, H * W, 3):                                        # planted exact ties
        y, x = divmod(n, W)
        i, j = sorted(torch.randperm(K, generator=g)[:2].tolist()) if K > 1 else (0, 0)
        acc[y, x, i] = acc[y, x, j] = 2.0
        if n % 2 and K > 2:
            acc[y, x, K - 1] = 2.0
    acc = acc.to(device)
    labels = torch.randint(0, K, (H, W), generator=g, dtype=torch.uint8)
    labels[0, :9] = 255                                                 # ignore_index
    labels[5, 3:11] = K                                                 # out of range
    labels = labels.to(device)
    pred, cm = F.scene_finalize(acc, K, labels, 255)
    want = acc[..., :K].argmax(-1)
    assert pred.dtype == torch.uint8 and torch.equal(pred.long(), want)
    valid = (labels < K) & (labels != 255)
    ref = torch.bincount(labels[valid].long() * K + want[valid], minlength=K * K).reshape(K, K)
    assert cm.dtype == torch.int64 and torch.equal(cm, ref)
    assert int(cm.sum()) == H * W - 9 - 8
    pred2, cm2 = F.scene_finalize(acc, K)
    assert torch.equal(pred2, pred) and int(cm2.abs().sum()) == 0 and cm2.shape == (K, K)


# ------------------------------------------------------------------ predictor
def make_model(name, device, engine=True):
    """Seed 0, running statistics moved by three training-mode forwards, a decisive head."""
    from ddlpc.models import UNet
    torch.manual_seed(0)
    model = UNet(**MODELS[name]).to(device)
    if engine:
        model.to_hip()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        model.train()
        for _ in range(3):
            model(torch.rand(2, 3, 32, 32, generator=g).to(device))
        model.conv_last.weight *= 100
    return model


def stock_copy(model, device):
    from ddlpc.models import UNet
    ref = UNet.from_config(model.cfg).to(device)
    ref.load_state_dict(model.state_dict())
    return ref


def decisive(proba, margin=1e-4):
    """Pixels whose top-two class probabilities ([K, H, W]) differ by more than ``margin``."""
    top = proba.topk(2, dim=0).values
    return (top[0] - top[1]) > margin


def check_predictor_fused_vs_unfused(device, model, H, W, tile, overlap, blend):
    from ddlpc.infer import ScenePredictor
    scene = rand_scene(H, W, 2, device)
    fused = ScenePredictor(model, tile, overlap, blend, window_batch=3)
    unfused = ScenePredictor(model, tile, overlap, blend, window_batch=3, fused=False)
    assert fused.fused and not unfused.fused
    K = fused.classes
    was = model.training
    acc_f, acc_u = fused.accumulate(scene), unfused.accumulate(scene)
    assert model.training == was                                        # mode restored
    err = rel_err(acc_f, acc_u)
    print(f"predictor {H}x{W} tile {tile} overlap {overlap} {blend}: acc rel_err {err:.3e}")
    assert err < 1e-4
    assert float(acc_f[..., K].min()) > 0                               # every pixel covered
    pu = acc_u[..., :K].permute(2, 0, 1) / acc_u[..., K]
    keep = decisive(pu)
    excluded = 1.0 - float(keep.float().mean())
    print(f"  excluded share {excluded:.4%}")
    assert excluded <= 0.01
    pred_f, cm = fused.predict(scene)
    assert cm is None and pred_f.dtype == torch.uint8 and pred_f.shape == (H, W)
    pred_u = acc_u[..., :K].argmax(-1).cpu()
    assert torch.equal(pred_f.long()[keep.cpu()], pred_u[keep.cpu()])
    assert torch.equal(fused.accumulate(scene), acc_f)                  # reproducible: no atomics
    assert torch.allclose(fused.proba(scene).sum(0), torch.ones(H, W, device=device), atol=1e-5)
    return err


def check_predictor_vs_fp32(device, model, H, W, tile, overlap):
    """The engine's class map agrees with the fp32 stock modules on at least the share of
    pixels stock bf16 autocast does, minus 0.01."""
    from ddlpc.infer import ScenePredictor
    scene = rand_scene(H, W, 2, device)
    ref = stock_copy(model, device)
    p32, _ = ScenePredictor(ref, tile, overlap, "cosine", window_batch=3).predict(scene)
    pac = ScenePredictor(ref, tile, overlap, "cosine", window_batch=3)
    pac.autocast = True
    pa, _ = pac.predict(scene)
    pe, _ = ScenePredictor(model, tile, overlap, "cosine", window_batch=3).predict(scene)
    agree_e = float((pe == p32).float().mean())
    agree_a = float((pa == p32).float().mean())
    print(f"vs fp32 {H}x{W}: engine {agree_e:.4f} autocast {agree_a:.4f}")
    assert agree_e >= agree_a - 0.01


def check_single_window_matches_forward(device, model):
    from ddlpc.infer import ScenePredictor
    scene = rand_scene(32, 32, 4, device)
    pred, _ = ScenePredictor(model, 32, 0, "cosine").predict(scene)
    x = (scene.float() / 255).permute(2, 0, 1)[None].contiguous()
    model.eval()
    with torch.no_grad():
        logits = model(x).float()[0]
    model.train()
    keep = decisive(torch.softmax(logits, 0)).cpu()
    assert 1.0 - float(keep.float().mean()) <= 0.01
    assert torch.equal(pred.long()[keep], logits.argmax(0).cpu()[keep])


def check_predictor_arguments(device, model):
    import pytest

    from ddlpc.infer import ScenePredictor, blend_weights, plan_windows
    for bad in [(64, 64, 32, 7), (64, 64, 32, 18), (64, 64, 32, -2), (0, 5, 32, 8)]:
        with pytest.raises(ValueError):
            plan_windows(*bad)
    with pytest.raises(ValueError):
        blend_weights(32, 8, "linear")
    with pytest.raises(ValueError):
        ScenePredictor(model, 34, 8)                                    # 34 % 2**depth != 0
    with pytest.raises(ValueError):
        ScenePredictor(stock_copy(model, device), 32, 8, fused=True)    # no engine attached
    with pytest.raises(ValueError):
        ScenePredictor(model, 32, 8).predict(torch.zeros(8, 8, 3))      # not uint8
