"""Bodies of the augmented-crop tests, written once and run on both kernel sets:
``test_crop_cpu.py`` passes ``"cpu"`` (the C++ kernels of ``csrc/cpu_ref.cpp``),
``test_crop_gpu.py`` passes ``"cuda"`` (the gfx950 kernels of ``csrc/data.hip``).

Every comparison of images, labels and params is exact: the recipe is integer arithmetic, one
IEEE division, separately rounded multiplies and adds, a clamp and one bf16 rounding."""
import json
import os

import numpy as np
import pytest
import torch

SCENE_SHAPES = lambda tile: [(5, 7), (16, 23), (40, 33), (tile, tile)]      # noqa: E731
GATHER_CASES = [(tile, in_ch, 8) for tile in (8, 24, 40) for in_ch in (1, 3, 4)] + \
               [(tile, 3, 4) for tile in (8, 24, 40)]
SAMPLES = [0, 7, 2**31 + 5, 2**40 + 3, 123456, 2**31 + 6, 1, 2]


def ops():
    from ddlpc.ops import _ext
    return _ext.ops()


def packed(shapes, in_ch, seed, device, classes=6):
    """Random scenes of the given sizes in the packed storage of ``crop_gather``."""
    g = np.random.default_rng(seed)
    px = [g.integers(0, 256, (h * w, in_ch), dtype=np.uint8) for h, w in shapes]
    lb = [g.integers(0, classes, (h * w,), dtype=np.uint8) for h, w in shapes]
    offs = np.concatenate([[0], np.cumsum([h * w for h, w in shapes])])[:-1]
    table = torch.tensor([(int(o), h, w) for o, (h, w) in zip(offs, shapes)], dtype=torch.int64)
    return (torch.from_numpy(np.concatenate(px)).to(device), torch.from_numpy(np.concatenate(lb)).to(device),
            table.to(device))


def assert_batch_equals_twin(x, y, scenes, labels, table, params, color, tile, in_ch):
    from ddlpc.data.scenes import crop_gather_reference
    xr, yr = crop_gather_reference(scenes, labels, table, params, color, tile)
    assert x.dtype == torch.bfloat16 and y.dtype == torch.int64
    assert x.shape[:3] == (params.shape[0], tile, tile) and y.shape == (params.shape[0], tile, tile)
    assert torch.equal(y.cpu(), yr)
    assert torch.equal(x[..., :in_ch].cpu(), xr.permute(0, 2, 3, 1).to(torch.bfloat16))
    assert not x[..., in_ch:].any()                                  # zero channel padding
    return xr, yr


# ------------------------------------------------------------------ 1. crop_gather geometry
def check_gather(device, tile, in_ch, cpad):
    shapes = SCENE_SHAPES(tile)
    scenes, labels, table = packed(shapes, in_ch, 3, device)
    n = len(shapes)
    rows = []
    for code in range(8):
        for k, (H, W) in enumerate(shapes):
            origins = [(0, 0), (-3, -2), (H - tile + 5, W - tile + 3)]   # inside / before / past the end
            if H >= tile and W >= tile:
                origins.append((H - tile, W - tile))
            if k == n - 1:
                origins = [(0, 0)]                                   # the tile-sized scene
            rows += [(k, y0, x0, code) for y0, x0 in origins]
    rows += [(n, 0, 0, 0), (-1, 1, 2, 3)]                            # no such scene
    rows.append((2, 1, 2, 8 + 5))                                    # code is masked with & 7
    params = torch.tensor(rows, dtype=torch.int32, device=device)
    x, y = ops().crop_gather(scenes, labels, table, params, None, tile, cpad)
    assert x.shape[-1] == cpad
    xr, yr = assert_batch_equals_twin(x, y, scenes, labels, table, params, None, tile, in_ch)
    bad = [i for i, r in enumerate(rows) if not 0 <= r[0] < n]
    assert len(bad) == 2
    for i in bad:
        assert not x[i].any() and bool((y[i] == -100).all())
    # the masked code equals code 5 of the same crop
    p5 = torch.tensor([(2, 1, 2, 5)], dtype=torch.int32, device=device)
    x5, y5 = ops().crop_gather(scenes, labels, table, p5, None, tile, cpad)
    assert torch.equal(x5[0], x[-1]) and torch.equal(y5[0], y[-1])
    # the eight codes are the symmetries of the square: code c of a crop is the numpy recipe
    # applied to its code 0 (independent of the twin's cutting)
    per_code = len(rows[:-3]) // 8
    x0, y0 = x[:per_code].cpu().float().numpy(), y[:per_code].cpu().numpy()
    seen = set()
    for code in range(8):
        xc = x[code * per_code:(code + 1) * per_code].cpu().float().numpy()
        yc = y[code * per_code:(code + 1) * per_code].cpu().numpy()
        ex, ey = x0, y0
        if code & 2:
            ex, ey = ex[:, ::-1], ey[:, ::-1]
        if code & 1:
            ex, ey = ex[:, :, ::-1], ey[:, :, ::-1]
        if code & 4:
            ex, ey = ex.swapaxes(1, 2), ey.swapaxes(1, 2)
        assert np.array_equal(xc, ex) and np.array_equal(yc, ey), code
        seen.add(yc.tobytes())
    assert len(seen) == 8


def check_far_origins(device):
    """Origins at and beyond +-2^30 (any int32 origin is accepted; y0 + a still fits an int): the
    scene is mirrored many periods away, as the numpy twin cuts it, on both backends."""
    tile, in_ch = 24, 3
    shapes = [(5, 7), (16, 23)]
    scenes, labels, table = packed(shapes, in_ch, 5, device)
    far = 1 << 30
    origins = [(far, -far), (far + 5, far + 3), (-far - 7, far), (3, far + 11), (-far, -2)]
    rows = [(k, y0, x0, code) for code in range(8) for k in range(2) for y0, x0 in origins]
    params = torch.tensor(rows, dtype=torch.int32, device=device)
    x, y = ops().crop_gather(scenes, labels, table, params, None, tile, 8)
    assert_batch_equals_twin(x, y, scenes, labels, table, params, None, tile, in_ch)
    assert bool((y >= 0).all())                                      # every row was read


def check_gather_rejects(device):
    scenes, labels, table = packed([(9, 9)], 3, 0, device)
    p = torch.zeros(2, 4, dtype=torch.int32, device=device)
    F = ops()
    F.crop_gather(scenes, labels, table, p, None, 4, 8)
    for bad in (lambda: F.crop_gather(scenes.float(), labels, table, p, None, 4, 8),
                lambda: F.crop_gather(scenes, labels[:-1], table, p, None, 4, 8),
                lambda: F.crop_gather(scenes, labels, table.int(), p, None, 4, 8),
                lambda: F.crop_gather(scenes, labels, table[:, :2].contiguous(), p, None, 4, 8),
                lambda: F.crop_gather(scenes, labels, table, p.long(), None, 4, 8),
                lambda: F.crop_gather(scenes, labels, table, p[:, :3].contiguous(), None, 4, 8),
                lambda: F.crop_gather(scenes, labels, table, p, torch.ones(3, 2, device=device), 4, 8),
                lambda: F.crop_gather(scenes, labels, table, p, torch.ones(2, 2, device=device).double(), 4, 8),
                lambda: F.crop_gather(scenes, labels, table, p, None, 0, 8),
                lambda: F.crop_gather(scenes, labels, table, p, None, 4, 2),
                lambda: F.crop_gather(torch.zeros(81, 9, dtype=torch.uint8, device=device), labels, table,
                                      p, None, 4, 8)):
        with pytest.raises(RuntimeError):
            bad()
    # a table row that does not lie inside the pixel buffer reads nothing
    wild = torch.tensor([[50, 9, 9], [0, -1, 9]], dtype=torch.int64, device=device)
    p2 = torch.tensor([[0, 0, 0, 0], [1, 0, 0, 0]], dtype=torch.int32, device=device)
    x, y = F.crop_gather(scenes, labels, wild, p2, None, 4, 8)
    assert not x.any() and bool((y == -100).all())


# ------------------------------------------------------------------ 2. colour
def check_color(device):
    tile, in_ch = 16, 3
    g = np.random.default_rng(5)
    img = np.concatenate([np.arange(256, dtype=np.uint8).repeat(3).reshape(256, 3),      # every byte value
                          g.integers(0, 256, (20 * 16 - 256, 3), dtype=np.uint8)])
    scenes = torch.from_numpy(img).to(device)
    labels = torch.from_numpy(g.integers(0, 6, (20 * 16,), dtype=np.uint8)).to(device)
    table = torch.tensor([[0, 20, 16]], dtype=torch.int64, device=device)
    col = [(1.0, 0.0), (2.5, 0.0), (1.0, -0.5), (0.7, 0.1), (1.3, -0.2), (0.3333333, 0.6666667),
           (1.0, 1.0), (0.0, 0.25), (1.1459, -0.0731)]
    params = torch.tensor([(0, 0, 0, i % 8) for i in range(len(col))], dtype=torch.int32, device=device)
    color = torch.tensor(col, dtype=torch.float32, device=device)
    x, y = ops().crop_gather(scenes, labels, table, params, color, tile, 8)
    xr, _ = assert_batch_equals_twin(x, y, scenes, labels, table, params, color, tile, in_ch)
    assert float(xr[1].max()) == 1.0 and float(xr[2].min()) == 0.0   # both clamps are reached
    mid = xr[3]
    assert 0.0 < float(mid.min()) and float(mid.max()) < 1.0         # ... and values in between
    assert bool((xr[6] == 1.0).all()) and bool((xr[7] == 0.25).all())
    # no colour == (gain 1, bias 0) == the plain path
    ident = torch.tensor([(1.0, 0.0)] * len(col), dtype=torch.float32, device=device)
    xa, ya = ops().crop_gather(scenes, labels, table, params, None, tile, 8)
    xb, yb = ops().crop_gather(scenes, labels, table, params, ident, tile, 8)
    assert torch.equal(xa, xb) and torch.equal(ya, yb) and torch.equal(ya, y)
    assert_batch_equals_twin(xa, ya, scenes, labels, table, params, None, tile, in_ch)


# ------------------------------------------------------------------ 3. identity == tile_gather
def check_identity_equals_tile_gather(device):
    g = np.random.default_rng(2)
    for T, C, cpad in ((24, 3, 8), (40, 4, 4), (33, 1, 8)):
        xs = torch.from_numpy(g.integers(0, 256, (9, T, T, C), dtype=np.uint8)).to(device)
        ys = torch.from_numpy(g.integers(0, 6, (9, T, T), dtype=np.uint8)).to(device)
        idx = torch.tensor([8, 0, 3, 3, 9, -1], dtype=torch.int64, device=device)
        xt, yt = ops().tile_gather(xs, ys, idx, cpad)
        table = torch.tensor([(k * T * T, T, T) for k in range(9)], dtype=torch.int64, device=device)
        params = torch.stack([idx, idx * 0, idx * 0, idx * 0], 1).to(torch.int32)
        xc, yc = ops().crop_gather(xs.reshape(-1, C), ys.reshape(-1), table, params, None, T, cpad)
        assert torch.equal(xc, xt) and torch.equal(yc, yt)


# ------------------------------------------------------------------ 4. crop_params
def _params_setup(device, tile=24):
    from ddlpc.data.scenes import crop_cum
    shapes = [(5, 7), (30, 41), (64, 50), (tile, tile), (26, 24)]
    table = torch.tensor([(0, h, w) for h, w in shapes], dtype=torch.int64)
    table[:, 0] = torch.tensor(np.concatenate([[0], np.cumsum([h * w for h, w in shapes])])[:-1])
    cum = torch.from_numpy(crop_cum(table.numpy(), tile))
    return shapes, table.to(device), cum.to(device)


def check_params(device):
    from ddlpc.data.scenes import crop_params_reference
    tile = 24
    shapes, table, cum = _params_setup(device, tile)
    assert cum.tolist() == [0, 1, 1 + 7 * 18, 127 + 41 * 27, 1235, 1238]
    idx = torch.tensor(SAMPLES + list(range(100, 164)), dtype=torch.int64, device=device)
    F = ops()
    for mode in (0, 1, 2):
        for gj, bj in ((0.0, 0.0), (0.25, 0.125), (0.1, 0.0)):
            p, c = F.crop_params(idx, cum, table, 11, tile, mode, gj, bj)
            pr, cr = crop_params_reference(idx, cum, table, 11, tile, mode, gj, bj)
            assert p.dtype == torch.int32 and p.shape == (idx.numel(), 4)
            assert c.dtype == torch.float32 and c.shape == (idx.numel(), 2)
            assert torch.equal(p.cpu(), pr) and torch.equal(c.cpu(), cr), (mode, gj, bj)
            for s, y0, x0, code in p.tolist():
                H, W = shapes[s]
                assert 0 <= y0 <= max(H - tile, 0) and 0 <= x0 <= max(W - tile, 0)
                assert 0 <= code <= (0, 3, 7)[mode]
            if gj == 0.0 and bj == 0.0:
                assert torch.equal(c.cpu(), torch.tensor([[1.0, 0.0]]).expand(idx.numel(), 2))
            else:
                assert float((c[:, 0] - 1).abs().max()) <= gj and float(c[:, 1].abs().max()) <= bj
                assert c[:, 0].unique().numel() > 32
    # a row depends on (seed, sample number) only: permuted and split batches, another seed
    p, c = F.crop_params(idx, cum, table, 11, tile, 2, 0.25, 0.125)
    perm = torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(0)).to(device)
    pp, cp = F.crop_params(idx[perm], cum, table, 11, tile, 2, 0.25, 0.125)
    assert torch.equal(pp, p[perm]) and torch.equal(cp, c[perm])
    for part in (slice(0, 5), slice(5, None)):
        ps, cs = F.crop_params(idx[part].contiguous(), cum, table, 11, tile, 2, 0.25, 0.125)
        assert torch.equal(ps, p[part]) and torch.equal(cs, c[part])
    p2, c2 = F.crop_params(idx, cum, table, 12, tile, 2, 0.25, 0.125)
    assert int((p2 != p).any(1).sum()) > idx.numel() // 2 and not torch.equal(c2, c)
    # the two halves of a 64-bit sample number both reach the key
    a = F.crop_params(torch.tensor([5, 2**32 + 5, 2**33 + 5], device=device), cum, table, 11, tile, 2, 0.25, 0.125)
    assert a[1].unique(dim=0).shape[0] == 3
    empty = F.crop_params(idx[:0], cum, table, 11, tile, 2, 0.0, 0.0)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 2)
    with pytest.raises(RuntimeError):
        F.crop_params(idx, cum[:-1].contiguous(), table, 11, tile, 2, 0.0, 0.0)
    with pytest.raises(RuntimeError):
        F.crop_params(idx, cum, table, 11, tile, 3, 0.0, 0.0)
    with pytest.raises(RuntimeError):
        F.crop_params(idx.int(), cum, table, 11, tile, 2, 0.0, 0.0)


# ------------------------------------------------------------------ 5. distribution
def check_distribution(device):
    from ddlpc.data.scenes import crop_cum
    tile = 16
    shapes = [(16, 16), (20, 47), (40, 33)]                          # 1, 160 and 450 origins
    table = torch.tensor([(0, h, w) for h, w in shapes], dtype=torch.int64, device=device)
    cum = torch.from_numpy(crop_cum(table.cpu().numpy(), tile)).to(device)
    w = np.diff(cum.cpu().numpy()).astype(np.float64)
    assert w.tolist() == [1.0, 160.0, 450.0]
    N = 4096
    idx = torch.arange(N, dtype=torch.int64, device=device)
    p = ops().crop_params(idx, cum, table, 1, tile, 2, 0.0, 0.0)[0].cpu().numpy()
    assert set(p[:, 3].tolist()) == set(range(8))
    assert set(ops().crop_params(idx, cum, table, 1, tile, 1, 0.0, 0.0)[0][:, 3].tolist()) == {0, 1, 2, 3}
    assert set(ops().crop_params(idx, cum, table, 1, tile, 0, 0.0, 0.0)[0][:, 3].tolist()) == {0}
    share = w / w.sum()
    for s in range(3):
        got = int((p[:, 0] == s).sum())
        sd = (N * share[s] * (1 - share[s])) ** 0.5
        assert abs(got - N * share[s]) <= 5 * sd, (s, got, N * share[s], sd)
    big = p[p[:, 0] == 2]
    assert big[:, 1].min() == 0 and big[:, 1].max() == 24 and big[:, 2].max() == 17


# ------------------------------------------------------------------ 6. the dataset
RAGGED = {"a0": (70, 90), "a1": (41, 33), "a2": (20, 75), "z8": (50, 37), "z9": (17, 40)}


def write_scenes(path, shapes=RAGGED, seed=0):
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    g = np.random.default_rng(seed)
    out = {}
    for stem, (h, w) in shapes.items():
        img = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        lab = g.integers(0, 6, (h, w), dtype=np.uint8)
        Image.fromarray(img).save(os.path.join(path, stem + ".png"))
        np.save(os.path.join(path, stem + "_label.npy"), lab)
        out[stem] = (img, lab)
    return out


def check_dataset(device, tmp_path):
    from ddlpc.data import SceneCropDataset, load_scenes
    from ddlpc.data.scenes import grid_origins
    tile = 32
    d = str(tmp_path / "scenes")
    raw = write_scenes(d)
    tr, te = load_scenes(d, 2)
    assert [x.shape[:2] for x, _ in tr] == [(70, 90), (41, 33), (20, 75)]
    assert [x.shape[:2] for x, _ in te] == [(50, 37), (17, 40)]
    assert np.array_equal(tr[1][0], raw["a1"][0]) and np.array_equal(te[1][1], raw["z9"][1])
    kw = dict(augment="d4", gain_jitter=0.2, bias_jitter=0.1, seed=4)
    eng, eng_te = SceneCropDataset.from_dir(d, tile, 2, layout="engine", **kw)
    eng.to_device(device), eng_te.to_device(device)
    ref, _ = SceneCropDataset.from_dir(d, tile, 2, layout="nchw", **kw)
    assert len(eng) == -(-(70 * 90 + 41 * 33 + 20 * 75) // tile ** 2) == 9
    assert len(SceneCropDataset(tr, tile, crops_per_epoch=21)) == 21
    idx = [0, 5, 8, 3]
    x, y = eng.get(idx)
    xp = x._ddlpc_nhwc
    assert xp.shape == (4, tile, tile, 8) and xp.dtype == torch.bfloat16 and x.shape == (4, 3, tile, tile)
    assert xp.device.type == torch.device(device).type and y.dtype == torch.int64
    x2, y2 = eng.get(torch.tensor(idx, device=device))               # device indices, same batch
    assert torch.equal(x2._ddlpc_nhwc, xp) and torch.equal(y2, y)
    xn, yn = ref.get(idx)                                            # the numpy twins
    assert xn.dtype == torch.float32 and xn.shape == (4, 3, tile, tile)
    assert torch.equal(y.cpu(), yn) and torch.equal(x.cpu(), xn.to(torch.bfloat16))
    eng.set_epoch(1), ref.set_epoch(1)
    x1, y1 = eng.get(idx)
    assert not torch.equal(x1._ddlpc_nhwc, xp)                       # another epoch, other crops
    assert torch.equal(x1.cpu(), ref.get(idx)[0].to(torch.bfloat16))
    # epoch e, sample i is virtual sample e * len + i
    assert torch.equal(eng.sample_numbers([2]).cpu(), torch.tensor([len(eng) + 2]))
    eng.set_epoch(0)
    x0, y0 = eng.get(idx)
    assert torch.equal(x0._ddlpc_nhwc, xp) and torch.equal(y0, y)
    with pytest.raises(IndexError):
        eng.get([len(eng)])
    # held-out scenes: a grid of plain windows that covers every pixel
    assert grid_origins(50, 37, tile) == [(0, 0), (0, 5), (18, 0), (18, 5)]
    assert grid_origins(17, 40, tile) == [(0, 0), (0, 8)]
    assert grid_origins(64, 32, tile) == [(0, 0), (32, 0)] and grid_origins(5, 7, tile) == [(0, 0)]
    assert len(eng_te) == 6
    rows = eng_te.params.cpu().tolist()
    for k, (img, lab) in enumerate(te):
        H, W = lab.shape
        cover = np.zeros((H, W), dtype=np.int64)
        for i, (s, y0, x0, code) in enumerate(rows):
            if s != k:
                continue
            assert code == 0 and 0 <= y0 <= max(H - tile, 0) and 0 <= x0 <= max(W - tile, 0)
            cover[y0:y0 + tile, x0:x0 + tile] += 1
            xw, yw = eng_te.get([i])
            h, w = min(tile, H - y0), min(tile, W - x0)
            assert np.array_equal(yw[0, :h, :w].cpu().numpy(), lab[y0:y0 + h, x0:x0 + w])
            want = (torch.from_numpy(img[y0:y0 + h, x0:x0 + w].copy()).float() / 255.0).to(torch.bfloat16)
            assert torch.equal(xw[0, :, :h, :w].permute(1, 2, 0).cpu(), want)
        assert cover.min() >= 1
    # a label map of another size
    bad = str(tmp_path / "bad")
    write_scenes(bad, {"s0": (20, 20), "s1": (12, 30)})
    np.save(os.path.join(bad, "s1_label.npy"), np.zeros((30, 12), dtype=np.uint8))
    with pytest.raises(ValueError):
        load_scenes(bad, 0)


def check_tiles_as_scenes(device, tmp_path):
    """A pre-cut tile set with ``augment="d4"`` serves only D4 images of its own tiles."""
    from ddlpc.data import SceneCropDataset, TileDataset
    T = 24
    d = str(tmp_path / "tiles")
    raw = write_scenes(d, {f"t{i}": (T, T) for i in range(5)}, seed=9)
    xs = np.stack([raw[f"t{i}"][0] for i in range(5)])
    ys = np.stack([raw[f"t{i}"][1] for i in range(5)])
    tiles, held = TileDataset.from_dir(d, 0)
    assert held is None and len(tiles) == 5
    ds = SceneCropDataset.from_tiles(tiles, T, crops_per_epoch=64, augment="d4",
                                     layout="engine", seed=2).to_device(device)
    p, c = ds.crop_rows(list(range(64)))
    assert c is None and not p[:, 1:3].any()                          # origin (0, 0) always
    assert set(p[:, 0].tolist()) == set(range(5)) and set(p[:, 3].tolist()) == set(range(8))
    images = {}
    for k in range(5):
        for code in range(8):
            a, b = xs[k], ys[k]
            if code & 2:
                a, b = a[::-1], b[::-1]
            if code & 1:
                a, b = a[:, ::-1], b[:, ::-1]
            if code & 4:
                a, b = a.swapaxes(0, 1), b.swapaxes(0, 1)
            images[(k, code)] = (torch.from_numpy(a.copy()).float().div(255.0).to(torch.bfloat16),
                                 torch.from_numpy(b.astype(np.int64)))
    x, y = ds.get(list(range(64)))
    for i, (k, _, _, code) in enumerate(p.tolist()):
        assert torch.equal(x[i].permute(1, 2, 0).cpu(), images[(k, code)][0])
        assert torch.equal(y[i].cpu(), images[(k, code)][1])


# ------------------------------------------------------------------ 7. training
def synthetic_scene(h_tiles, w_tiles, H, W, first, tile=64, seed=3):
    """A scene pasted together from ``render_synthetic`` tiles (classes separable by colour,
    so it stays learnable under any symmetry), cropped to H x W."""
    from ddlpc.data.datasets import render_synthetic
    x, y = render_synthetic(list(range(first, first + h_tiles * w_tiles)), seed, 6, 3, tile, 2)
    img = (x.permute(0, 2, 3, 1) * 255.0).round().to(torch.uint8).numpy()
    img = img.reshape(h_tiles, w_tiles, tile, tile, 3).transpose(0, 2, 1, 3, 4).reshape(h_tiles * tile, w_tiles * tile, 3)
    lab = y.to(torch.uint8).numpy().reshape(h_tiles, w_tiles, tile, tile).transpose(0, 2, 1, 3)
    lab = lab.reshape(h_tiles * tile, w_tiles * tile)
    return img[:H, :W].copy(), lab[:H, :W].copy()


def write_training_scenes(path):
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    for name, args in (("s0", (3, 2, 180, 128, 0)), ("s1", (2, 3, 100, 170, 6)), ("s2", (2, 2, 90, 110, 12))):
        img, lab = synthetic_scene(*args)
        Image.fromarray(img).save(os.path.join(path, name + ".png"))
        np.save(os.path.join(path, name + "_label.npy"), lab)


def train_cfg(tmp_path, data_dir, **kw):
    from ddlpc.config import ModelConfig, TrainConfig
    base = dict(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=4, test_holdout=1, impl="hip",
                data="scene_dir", data_dir=data_dir, crops_per_epoch=16, augment="d4", gain_jitter=0.1,
                bias_jitter=0.05, epochs=2, log_every=1, log_dir=str(tmp_path / "log"), ckpt_dir=None,
                timeout_s=120)
    base.update(kw)
    return TrainConfig(**base)


def check_training(device, tmp_path, model):
    """fit() + validate() on a directory of unequal scenes with D4 and colour jitter, and the
    crop stream across a resume: two epochs straight through == one epoch, checkpoint, resume,
    one epoch, bit for bit."""
    from ddlpc.data import SceneCropDataset
    from ddlpc.train.trainer import Trainer
    d = str(tmp_path / "scenes")
    write_training_scenes(d)
    tr = Trainer(train_cfg(tmp_path / "full", d, model=model), device=device)
    assert isinstance(tr.train_set, SceneCropDataset) and len(tr.train_set) == 16
    assert isinstance(tr.test_set, SceneCropDataset) and len(tr.test_set) == 4      # 90 x 110: 2 x 2
    x, _ = tr.train_set.get([0, 1])
    assert getattr(x, "_ddlpc_nhwc", None) is not None and x._ddlpc_nhwc.device.type == torch.device(device).type
    m = tr.fit()
    v = tr.validate()
    full = tr.flat.param_buf.clone()
    tr.close()
    assert m["steps"] == 8 and np.isfinite(m["loss"])
    assert set(v) >= {"val_loss", "val_pixel_acc", "val_iou", "val_miou"}
    assert np.isfinite(v["val_loss"]) and 0.0 <= v["val_pixel_acc"] <= 1.0
    recs = [json.loads(s) for s in (tmp_path / "full" / "log" / "metrics.jsonl").read_text().splitlines()]
    losses = [r["loss"] for r in recs if "images_per_s" in r]
    assert len(losses) == 8 and losses[-1] < losses[0], losses
    ck = str(tmp_path / "ck")
    t1 = Trainer(train_cfg(tmp_path / "p1", d, model=model, epochs=1, ckpt_dir=ck, log_dir=None), device=device)
    t1.fit()
    assert (t1.epoch, t1.step_count) == (1, 4)
    t1.close()
    t2 = Trainer(train_cfg(tmp_path / "p2", d, model=model, epochs=2, ckpt_dir=ck, resume="auto", log_dir=None),
                 device=device)
    assert t2.epoch == 1
    t2.fit()
    assert t2.step_count == 8 and t2.train_set.epoch == 1
    assert torch.equal(t2.flat.param_buf, full)
    t2.close()


# ------------------------------------------------------------------ 8. config and CLI
def check_config_and_cli(tmp_path):
    import argparse
    from ddlpc.config import ModelConfig, TrainConfig, add_config_args, config_from_args
    c = TrainConfig(data="scene_dir", data_dir="/x", crops_per_epoch=40, augment="flip", gain_jitter=0.2,
                    bias_jitter=0.05).validate()
    assert c.augmented and not TrainConfig().augmented
    assert TrainConfig(gain_jitter=0.1).augmented and TrainConfig(bias_jitter=0.1).augmented
    d = TrainConfig().to_dict()
    assert (d["crops_per_epoch"], d["augment"], d["gain_jitter"], d["bias_jitter"]) == (0, "none", 0.0, 0.0)
    c2 = TrainConfig.from_dict(json.loads(json.dumps(c.to_dict())))
    assert c2 == c
    p = str(tmp_path / "c.json")
    c.save(p)
    assert TrainConfig.load(p) == c
    y = str(tmp_path / "c.yaml")
    with open(y, "w") as f:
        f.write("data: scene_dir\ndata_dir: /x\ncrops_per_epoch: 40\naugment: flip\n"
                "gain_jitter: 0.2\nbias_jitter: 0.05\n")
    assert TrainConfig.load(y) == c
    ap = add_config_args(argparse.ArgumentParser())
    a = ap.parse_args(["--data", "scene_dir", "--data-dir", "/x", "--crops-per-epoch", "40", "--augment", "flip",
                       "--gain-jitter", "0.2", "--bias-jitter", "0.05"])
    assert config_from_args(a) == c
    a = ap.parse_args(["--config", y, "--augment", "d4", "--bias-jitter", "0"])
    c3 = config_from_args(a)
    assert (c3.augment, c3.bias_jitter, c3.gain_jitter, c3.crops_per_epoch) == ("d4", 0.0, 0.2, 40)
    for bad in (dict(augment="rot90"), dict(gain_jitter=-0.1), dict(bias_jitter=1.5), dict(crops_per_epoch=-1),
                dict(data="scenes")):
        with pytest.raises(ValueError):
            TrainConfig(**bad).validate()
    tiles = dict(data="vaihingen_dir", data_dir="/x")
    for aug in (dict(augment="d4"), dict(gain_jitter=0.1), dict(bias_jitter=0.1), dict(crops_per_epoch=8),
                dict(data="scene_dir")):
        TrainConfig(**dict(tiles, **aug)).validate()
        with pytest.raises(ValueError):
            TrainConfig(model=ModelConfig(dims=3), **dict(tiles, **aug)).validate()
        if "data" not in aug:
            with pytest.raises(ValueError):                          # rendered tiles are not cropped
                TrainConfig(data="synthetic", **aug).validate()
    TrainConfig(model=ModelConfig(dims=3), **tiles).validate()
    TrainConfig(model=ModelConfig(dims=3)).validate()
