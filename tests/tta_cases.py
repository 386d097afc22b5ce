"""Bodies of the test-time-augmentation tests, written once and run on both kernel sets:
``test_tta_cpu.py`` passes ``"cpu"`` (the C++ kernels of ``csrc/cpu_ref.cpp``),
``test_tta_gpu.py`` passes ``"cuda"`` (the gfx950 kernels).

The symmetry convention is ``crop_gather``'s: for code ``c`` network-side pixel ``(oy, ox)``
is window-frame pixel ``(a, b) = (oy, ox)``; ``c & 4``: swap ``a``, ``b``; ``c & 2``:
``a = tile - 1 - a``; ``c & 1``: ``b = tile - 1 - b``.  ``frame_index`` below writes it out
on its own (it does not import the predictor's maps)."""
import functools

import pytest
import torch

from predict_cases import HEAD_CASES, HEAD_ORIGINS, PREDICTOR_SHAPES, _bn4, decisive, ops, rand_scene, rel_err

GATHER_CASES = [(40, 27, 16), (40, 27, 40), (5, 7, 16), (5, 7, 40)]
GATHER_CODES = [[c] for c in range(8)] + [[0, 1, 2, 3], list(range(8)), [6, 1, 4]]
CHANNEL_CASES = [(1, 1), (3, 4), (5, 8), (8, 8)]                        # (in_ch, cpad)
HEAD_CODES = [list(range(8)), [0, 1, 2, 3], [5]]
TTA_SHAPES = PREDICTOR_SHAPES + [(48, 48, 32, 16)]
EQUIVARIANCE_SHAPES = [(32, 32, 32, 0), (48, 48, 32, 16)]


def frame_index(tile, code, device):
    """-> (a, b), int64 [tile, tile]: the window-frame pixel of network-side pixel (oy, ox)."""
    oy, ox = torch.meshgrid(torch.arange(tile, device=device), torch.arange(tile, device=device),
                            indexing="ij")
    a, b = oy, ox
    if code & 4:
        a, b = b, a
    if code & 2:
        a = tile - 1 - a
    if code & 1:
        b = tile - 1 - b
    return a, b


def codes_tensor(codes, device):
    return torch.tensor(codes, dtype=torch.int32, device=device)


# ------------------------------------------------------------------ 1. window_gather with codes
@functools.lru_cache(maxsize=None)
def _plain_windows(device, H, W, tile):
    """(origins, origins tensor, fp32 reference windows [N, tile, tile, 8]) — computed once."""
    from ddlpc.infer import plan_windows, reflect
    scene = rand_scene(H, W, 1, device)
    origins = [o for g in plan_windows(H, W, tile, (tile // 2) & ~1) for o in g]
    origins += [(-tile + 1, -tile + 1), (H - 1, W - 1), (-3, W - 2), (H - 2, -5)]   # all four sides
    ref = torch.zeros(len(origins), tile, tile, 8, device=device)
    for n, (y0, x0) in enumerate(origins):
        iy = torch.tensor([reflect(y0 + t, H) for t in range(tile)], device=device)
        ix = torch.tensor([reflect(x0 + t, W) for t in range(tile)], device=device)
        ref[n, :, :, :3] = scene.index_select(0, iy).index_select(1, ix).float() / 255
    return scene, origins, torch.tensor(origins, dtype=torch.int32, device=device), ref.bfloat16()


def check_window_gather_codes(device, H, W, tile):
    scene, origins, o, plain = _plain_windows(device, H, W, tile)
    F = ops()
    N = len(origins)
    base = F.window_gather(scene, o, tile, 8)
    assert torch.equal(base, plain)
    assert torch.equal(F.window_gather(scene, o, tile, 8, codes_tensor([0], device)), base)
    for codes in GATHER_CODES:
        got = F.window_gather(scene, o, tile, 8, codes_tensor(codes, device))
        S = len(codes)
        assert got.dtype == torch.bfloat16 and got.shape == (N * S, tile, tile, 8)
        got = got.reshape(N, S, tile, tile, 8)
        for j, c in enumerate(codes):
            a, b = frame_index(tile, c, device)
            assert torch.equal(got[:, j], plain[:, a, b]), (codes, j)


def check_window_gather_channels(device, in_ch, cpad):
    """Every (in_ch, cpad), not only the 16-byte store of cpad = 8 with 3 channels: a 5 x 7
    scene (windows of 40 reflect several times), tile 40 = 2 x 2 blocks of 32 with the second
    ragged; without codes against the torch expression, under codes against the index map."""
    from ddlpc.infer import reflect
    H, W, tile = 5, 7, 40
    origins = [(-39, -39), (4, 6), (-3, 5)]
    scene = rand_scene(H, W, 3, device, in_ch)
    o = torch.tensor(origins, dtype=torch.int32, device=device)
    ref = torch.zeros(len(origins), tile, tile, cpad, device=device)
    for n, (y0, x0) in enumerate(origins):
        iy = torch.tensor([reflect(y0 + t, H) for t in range(tile)], device=device)
        ix = torch.tensor([reflect(x0 + t, W) for t in range(tile)], device=device)
        ref[n, :, :, :in_ch] = scene.index_select(0, iy).index_select(1, ix).float() / 255
    plain = ref.bfloat16()
    F = ops()
    got = F.window_gather(scene, o, tile, cpad)
    assert got.dtype == torch.bfloat16 and got.shape == (len(origins), tile, tile, cpad)
    assert torch.equal(got, plain)
    codes = [6, 1, 4]
    got = F.window_gather(scene, o, tile, cpad, codes_tensor(codes, device))
    assert got.dtype == torch.bfloat16 and got.shape == (len(origins) * len(codes), tile, tile, cpad)
    got = got.reshape(len(origins), len(codes), tile, tile, cpad)
    for j, c in enumerate(codes):
        a, b = frame_index(tile, c, device)
        assert torch.equal(got[:, j], plain[:, a, b]), (codes, j)


# ------------------------------------------------------------------ 2. head_predict_accum with codes
def _slice_add(add, frame, w2, origins, tile, K):
    """add[y0 + a, x0 + b, :K] = w2 * frame[n, a, b], add[.., K] = w2 inside the scene."""
    H, W = add.shape[0], add.shape[1]
    for n, (y0, x0) in enumerate(origins):
        ys, xs, ye, xe = max(0, -y0), max(0, -x0), min(tile, H - y0), min(tile, W - x0)
        add[y0 + ys:y0 + ye, x0 + xs:x0 + xe, :K] = frame[n, ys:ye, xs:xe] * w2[ys:ye, xs:xe, None]
        add[y0 + ys:y0 + ye, x0 + xs:x0 + xe, K] = w2[ys:ye, xs:xe]


def check_head_predict_accum_codes(device, C, K, blend):
    """rel_err of the added part < 1e-4 against fp32 torch on the same bf16 activation: the
    tolerance of ``check_head_predict_accum`` (the same arithmetic plus an S-term sum)."""
    from ddlpc.infer import acc_channels, blend_weights
    F = ops()
    H, W, tile = 40, 27, 16
    KA = acc_channels(K)
    B = len(HEAD_ORIGINS)
    g = torch.Generator().manual_seed(7)
    wh = (torch.randn(K, C, generator=g) * 0.3).to(device)
    bh = (torch.randn(K, generator=g) * 0.1).to(device)
    fill = torch.randn(H, W, KA, generator=g).to(device)
    win = blend_weights(tile, 8, blend).to(device)
    w2 = win[:, None] * win[None, :]
    o = torch.tensor(HEAD_ORIGINS, dtype=torch.int32, device=device)
    bn4 = _bn4(C, device)
    for codes in HEAD_CODES:
        S = len(codes)
        ct = codes_tensor(codes, device)
        a = torch.relu(torch.randn(B * S, tile, tile, C, generator=g)).bfloat16().to(device)
        acc = fill.clone()
        F.head_predict_accum(a, wh, bh, o, win, acc, None, ct)
        # fp32 torch: the S softmaxes un-mapped into the window frame, averaged, weighted
        p = torch.softmax(a.float() @ wh.t() + bh, dim=-1).reshape(B, S, tile, tile, K)
        frame = torch.zeros(B, tile, tile, K, device=device)
        for j, c in enumerate(codes):
            ia, ib = frame_index(tile, c, device)
            un = torch.empty(B, tile, tile, K, device=device)
            un[:, ia, ib] = p[:, j]
            frame += un
        frame /= S
        add = torch.zeros(H, W, KA, device=device)
        _slice_add(add, frame, w2, HEAD_ORIGINS, tile, K)
        touched = add[..., K] != 0
        assert 0 < int(touched.sum()) < H * W
        err = rel_err(acc - fill, add)
        print(f"head_predict_accum codes={codes} C={C} K={K} {blend}: rel_err {err:.3e}")
        assert err < 1e-4
        assert torch.equal(acc[..., K + 1:], fill[..., K + 1:])         # channels above K
        assert torch.equal(acc[~touched], fill[~touched])               # uncovered / zero weight
        again = fill.clone()
        F.head_predict_accum(a, wh, bh, o, win, again, None, ct)
        assert torch.equal(again, acc)                                  # reproducible: no atomics
        # deferred BatchNorm: bit-identical to the call on the materialised activation
        y = torch.randn(B * S, tile, tile, C, generator=g).bfloat16().to(device)
        act = F.bn_relu_apply(y, bn4, False)[0]
        acc_d, acc_m = fill.clone(), fill.clone()
        F.head_predict_accum(y, wh, bh, o, win, acc_d, bn4, ct)
        F.head_predict_accum(act, wh, bh, o, win, acc_m, None, ct)
        assert torch.equal(acc_d, acc_m)
        assert not torch.equal(acc_d, fill)
    # codes = [0] is the codes-free call, bit for bit (plain and deferred BatchNorm)
    a = torch.relu(torch.randn(B, tile, tile, C, generator=g)).bfloat16().to(device)
    zero = codes_tensor([0], device)
    for bn in (None, bn4):
        acc_0, acc_n = fill.clone(), fill.clone()
        F.head_predict_accum(a, wh, bh, o, win, acc_0, bn, zero)
        F.head_predict_accum(a, wh, bh, o, win, acc_n, bn)
        assert torch.equal(acc_0, acc_n)
        assert not torch.equal(acc_0, fill)


# ------------------------------------------------------------------ 3. the two kernels, no network
def check_round_trip(device):
    """The gathered views themselves as the activation (C = 8, K = 3): the head is pointwise, so
    every view contributes the same softmax to a scene pixel and the result is the plain gather
    + accumulate up to the rounding of the S-term mean (rel_err < 1e-6; a map that differs
    between the two kernels fails at order 1)."""
    from ddlpc.infer import acc_channels, blend_weights
    F = ops()
    H, W, tile, C, K = 40, 27, 16, 8, 3
    scene = rand_scene(H, W, 9, device)
    g = torch.Generator().manual_seed(13)
    wh = torch.randn(K, C, generator=g).to(device)
    bh = (torch.randn(K, generator=g) * 0.1).to(device)
    win = blend_weights(tile, 8, "cosine").to(device)
    o = torch.tensor(HEAD_ORIGINS, dtype=torch.int32, device=device)
    plain = torch.zeros(H, W, acc_channels(K), device=device)
    F.head_predict_accum(F.window_gather(scene, o, tile, 8), wh, bh, o, win, plain)
    assert float(plain[..., K].max()) > 0
    for codes in GATHER_CODES:
        ct = codes_tensor(codes, device)
        acc = torch.zeros_like(plain)
        F.head_predict_accum(F.window_gather(scene, o, tile, 8, ct), wh, bh, o, win, acc, None, ct)
        err = rel_err(acc, plain)
        print(f"round trip codes={codes}: rel_err {err:.3e}")
        assert err < 1e-6


# ------------------------------------------------------------------ 4. predictor, fused against unfused
def check_predictor_tta(device, model, H, W, tile, overlap, tta, window_batch=16):
    from ddlpc.infer import TTA_CODES, ScenePredictor
    scene = rand_scene(H, W, 2, device)
    fused = ScenePredictor(model, tile, overlap, "cosine", window_batch=window_batch, tta=tta)
    unfused = ScenePredictor(model, tile, overlap, "cosine", window_batch=window_batch, fused=False, tta=tta)
    assert fused.fused and not unfused.fused
    K, S = fused.classes, len(TTA_CODES[tta])
    was = model.training
    acc_f, acc_u = fused.accumulate(scene), unfused.accumulate(scene)
    assert model.training == was
    s = tile - overlap
    assert fused.windows == unfused.windows == -(-H // s) * -(-W // s)
    assert fused.inputs == unfused.inputs == fused.windows * S
    err = rel_err(acc_f, acc_u)
    print(f"predictor tta={tta} {H}x{W} tile {tile} overlap {overlap} batch {window_batch}: "
          f"acc rel_err {err:.3e}")
    assert err < 1e-4
    assert float(acc_f[..., K].min()) > 0                               # every pixel covered
    keep = decisive(unfused.proba_of(acc_u))
    excluded = 1.0 - float(keep.float().mean())
    print(f"  excluded share {excluded:.4%}")
    assert excluded <= 0.01
    pred_f, cm = fused.finalize(acc_f)
    assert cm is None and pred_f.dtype == torch.uint8 and pred_f.shape == (H, W)
    pred_u = acc_u[..., :K].argmax(-1).cpu()
    assert torch.equal(pred_f.long()[keep.cpu()], pred_u[keep.cpu()])
    assert torch.equal(fused.accumulate(scene), acc_f)                  # reproducible: no atomics
    assert torch.allclose(fused.proba(scene).sum(0), torch.ones(H, W, device=device), atol=1e-5)
    return err


# ------------------------------------------------------------------ 5. equivariance
def _transformed(scene, g):
    """Scene under symmetry g (square): out[oy, ox] = scene[a, b]; and the index (a, b)."""
    a, b = frame_index(scene.shape[0], g, scene.device)
    return scene[a, b].contiguous(), (a, b)


def check_equivariance(device, model, H, tile, overlap, tta, group):
    """Predicting the transformed scene gives the transformed accumulator: with the whole
    symmetry group averaged the network sees the same set of inputs in another order, so only
    the order of the S-term sums differs (fp32 CPU probe: 2e-8 .. 5e-8; bound 1e-4).  Without
    test-time augmentation the same comparison measured 0.13 .. 0.22 (asserted > 1e-2)."""
    from ddlpc.infer import ScenePredictor
    assert H % (tile - overlap) == 0                                    # a symmetric plan
    scene = rand_scene(H, H, 6, device)
    sp = ScenePredictor(model, tile, overlap, "cosine", window_batch=16, tta=tta)
    plain = ScenePredictor(model, tile, overlap, "cosine", window_batch=16)
    acc, acc_plain = sp.accumulate(scene), plain.accumulate(scene)
    for g in group:
        sg, (a, b) = _transformed(scene, g)
        err = rel_err(sp.accumulate(sg), acc[a, b])
        err_plain = rel_err(plain.accumulate(sg), acc_plain[a, b])
        print(f"equivariance tta={tta} {H}x{H} tile {tile} overlap {overlap} g={g}: "
              f"rel_err {err:.3e} (tta=none: {err_plain:.3e})")
        assert err < 1e-4
        assert err_plain > 1e-2


# ------------------------------------------------------------------ 6. tta="none" is the default path
def check_none_is_default(device, model):
    from ddlpc.infer import ScenePredictor
    scene = rand_scene(70, 52, 2, device)
    for fused in (True, False):
        a = ScenePredictor(model, 32, 16, "cosine", window_batch=3, fused=fused, tta="none")
        b = ScenePredictor(model, 32, 16, "cosine", window_batch=3, fused=fused)
        assert torch.equal(a.accumulate(scene), b.accumulate(scene))
        assert a.windows == b.windows == a.inputs == b.inputs


def check_none_counters(device, model):
    """Without test-time augmentation a pass is ``window_batch`` windows, one input each, and the
    accumulator is that of the codes-free ops called batch by batch in the plan's order."""
    from ddlpc.data.datasets import engine_input
    from ddlpc.infer import ScenePredictor, plan_windows
    H, W, tile, overlap, batch = 70, 52, 32, 16, 3
    scene = rand_scene(H, W, 2, device)
    groups = plan_windows(H, W, tile, overlap)
    sp = ScenePredictor(model, tile, overlap, "cosine", window_batch=batch, tta="none")
    acc = sp.accumulate(scene)
    assert sp.windows == sp.inputs == sum(len(g) for g in groups)
    unfused = ScenePredictor(model, tile, overlap, "cosine", window_batch=batch, fused=False, tta="none")
    unfused.accumulate(scene)
    assert unfused.windows == unfused.inputs == sp.windows
    F, eng = ops(), model._engine
    win = sp.win.to(device)
    want = torch.zeros_like(acc)
    was = model.training
    model.eval()
    with torch.no_grad():
        for g in groups:
            for i in range(0, len(g), batch):
                o = torch.tensor(g[i:i + batch], dtype=torch.int32, device=device)
                a, s = eng.features(engine_input(F.window_gather(scene, o, tile, 8), 3), defer_last=True)
                wh, bh = eng._head_params()
                F.head_predict_accum(a, wh.detach().contiguous(), bh.detach().contiguous(), o, win, want, s)
    model.train(was)
    assert torch.equal(acc, want)


# ------------------------------------------------------------------ 7. arguments
def check_arguments(device, model):
    from ddlpc.infer import ScenePredictor
    F = ops()
    scene = rand_scene(20, 20, 1, device)
    o = torch.zeros(1, 2, dtype=torch.int32, device=device)
    a = torch.zeros(2, 16, 16, 32, dtype=torch.bfloat16, device=device)
    wh, bh = torch.zeros(6, 32, device=device), torch.zeros(6, device=device)
    win = torch.ones(16, device=device)
    acc = torch.zeros(20, 20, 8, device=device)
    F.window_gather(scene, o, 16, 8, codes_tensor([3, 4], device))
    F.head_predict_accum(a, wh, bh, o, win, acc, None, codes_tensor([3, 4], device))
    # a codes tensor rewritten in place is read again (the bindings remember a checked list)
    ct = codes_tensor([3, 4], device)
    x34 = F.window_gather(scene, o, 16, 8, ct)
    ct.copy_(codes_tensor([4, 3], device))
    assert torch.equal(F.window_gather(scene, o, 16, 8, ct), x34.flip(0))
    ct[1] = 4
    with pytest.raises(RuntimeError):
        F.window_gather(scene, o, 16, 8, ct)
    bad = [codes_tensor([1, 1], device),                                # duplicate
           codes_tensor([0, 8], device),                                # out of range
           codes_tensor([-1, 2], device),
           codes_tensor([0, 1], device).long(),                         # int64
           codes_tensor([0, 1, 2, 3, 4, 5, 6, 7, 0], device),           # S = 9
           codes_tensor([], device),                                    # S = 0
           codes_tensor([[0, 1]], device)]                              # not 1-D
    for ct in bad:
        with pytest.raises(RuntimeError):
            F.window_gather(scene, o, 16, 8, ct)
        with pytest.raises(RuntimeError):
            F.head_predict_accum(a, wh, bh, o, win, acc, None, ct)
    with pytest.raises(RuntimeError):                                   # a.size(0) != B * S
        F.head_predict_accum(a, wh, bh, o, win, acc, None, codes_tensor([0, 1, 2], device))
    with pytest.raises(RuntimeError):
        F.head_predict_accum(a, wh, bh, torch.zeros(2, 2, dtype=torch.int32, device=device), win, acc,
                             None, codes_tensor([0, 1], device))
    if device != "cpu":                                                 # codes on another device
        with pytest.raises(RuntimeError):
            F.window_gather(scene, o, 16, 8, codes_tensor([0, 1], "cpu"))
        with pytest.raises(RuntimeError):
            F.head_predict_accum(a, wh, bh, o, win, acc, None, codes_tensor([0, 1], "cpu"))
    with pytest.raises(ValueError):
        ScenePredictor(model, 32, 8, tta="rot")

