"""Bodies of the warped-crop tests (random zoom and rotation), written once and run on both
kernel sets: ``test_warp_cpu.py`` passes ``"cpu"`` (the C++ kernels of ``csrc/cpu_ref.cpp``),
``test_warp_gpu.py`` passes ``"cuda"`` (the gfx950 kernels of ``csrc/data.hip``).

Every comparison of images, labels and params is exact: the recipe is 16.16 fixed-point
integer arithmetic, separately rounded float32 multiplies, adds and subtractions, one IEEE
division, a clamp and one bf16 rounding."""
import numpy as np
import pytest
import torch

from crop_cases import (SAMPLES, SCENE_SHAPES, _params_setup, ops, packed, train_cfg, write_scenes,
                        write_training_scenes)

ONE = 65536
GATHER_CASES = [(tile, in_ch, 8) for tile in (8, 24, 40) for in_ch in (1, 3, 4)] + \
               [(tile, 3, 4) for tile in (8, 24, 40)]


def centre(o, tile):
    """16.16 centre of the unit-scale crop with origin ``o``."""
    return (2 * o + tile - 1) * 32768


def wrows(rows, device):
    return torch.tensor(rows, dtype=torch.int64, device=device).reshape(-1, 6)


def assert_batch_equals_twin(x, y, scenes, labels, table, wparams, color, tile, in_ch):
    from ddlpc.data.scenes import warp_gather_reference
    xr, yr = warp_gather_reference(scenes, labels, table, wparams, color, tile)
    assert x.dtype == torch.bfloat16 and y.dtype == torch.int64
    assert x.shape[:3] == (wparams.shape[0], tile, tile) and y.shape == (wparams.shape[0], tile, tile)
    assert torch.equal(y.cpu(), yr)
    assert torch.equal(x[..., :in_ch].cpu(), xr.permute(0, 2, 3, 1).to(torch.bfloat16))
    assert not x[..., in_ch:].any()                                  # zero channel padding
    return xr, yr


def crop_origins(shapes, tile):
    """(scene, y0, x0) triples: inside the scene, before its start, past its end."""
    out = []
    for k, (H, W) in enumerate(shapes):
        origins = [(0, 0), (-3, -2), (H - tile + 5, W - tile + 3)]
        if H >= tile and W >= tile:
            origins.append((H - tile, W - tile))
        if k == len(shapes) - 1:
            origins = [(0, 0)]                                       # the tile-sized scene
        out += [(k, y0, x0) for y0, x0 in origins]
    return out


# ------------------------------------------------------------------ 1. identity == crop_gather
def check_identity(device, tile, in_ch, cpad):
    shapes = SCENE_SHAPES(tile)
    scenes, labels, table = packed(shapes, in_ch, 3, device)
    crops = [(k, y0, x0, code) for code in range(8) for k, y0, x0 in crop_origins(shapes, tile)]
    params = torch.tensor(crops, dtype=torch.int32, device=device)
    wp = wrows([(k, centre(y0, tile), centre(x0, tile), code, ONE, 0) for k, y0, x0, code in crops], device)
    color = torch.tensor([(1.0 + 0.01 * (i % 7), 0.02 * (i % 5) - 0.04) for i in range(len(crops))],
                         dtype=torch.float32, device=device)
    for col in (None, color):
        xc, yc = ops().crop_gather(scenes, labels, table, params, col, tile, cpad)
        xw, yw = ops().warp_gather(scenes, labels, table, wp, col, tile, cpad)
        assert xw.shape == xc.shape and xw.dtype == xc.dtype and yw.dtype == yc.dtype
        assert torch.equal(xw, xc) and torch.equal(yw, yc)


# ------------------------------------------------------------------ 2. quarter turns
def check_quarter_turns(device, tile, in_ch, cpad):
    shapes = SCENE_SHAPES(tile)
    scenes, labels, table = packed(shapes, in_ch, 4, device)
    crops = crop_origins(shapes, tile)
    for (A, Bm), code in (((0, ONE), 5), ((-ONE, 0), 3), ((0, -ONE), 6)):
        params = torch.tensor([(k, y0, x0, code) for k, y0, x0 in crops], dtype=torch.int32, device=device)
        wp = wrows([(k, centre(y0, tile), centre(x0, tile), 0, A, Bm) for k, y0, x0 in crops], device)
        xc, yc = ops().crop_gather(scenes, labels, table, params, None, tile, cpad)
        xw, yw = ops().warp_gather(scenes, labels, table, wp, None, tile, cpad)
        assert torch.equal(xw, xc) and torch.equal(yw, yc), (A, Bm, code)


# ------------------------------------------------------------------ 3. the numpy twin
def random_rows(shapes, tile, seed, count=96):
    """Rows across zoom 0.25 .. 4 (steps ONE / 4 .. 4 ONE), arbitrary (A, Bm), fractional
    centres, overhang (centres from two tiles before the scene to two tiles past it), every
    code; the first rows pin the extremes."""
    g = np.random.default_rng(seed)
    n = len(shapes)
    rows = [(0, 12345, -54321, 0, ONE // 4, 0), (1, 5 * ONE + 1, 7 * ONE + 65535, 7, 4 * ONE, 0),
            (2, -3 * ONE, 9 * ONE + 32768, 5, -2 ** 20, 2 ** 20), (n - 1, 32768, 32767, 2, 0, 0),
            (1, 2 ** 46 - 1, -(2 ** 46 - 1), 3, 46341, -46341), (2, 20 * ONE, 16 * ONE, 8 + 6, 50000, 23456)]
    while len(rows) < count:
        k = int(g.integers(0, n))
        H, W = shapes[k]
        step = ONE * 4.0 ** g.uniform(-1, 1)
        th = g.uniform(-np.pi, np.pi)
        rows.append((k, int(g.integers(-2 * tile * ONE, (H + 2 * tile) * ONE)),
                     int(g.integers(-2 * tile * ONE, (W + 2 * tile) * ONE)), len(rows) % 8,
                     int(np.rint(step * np.cos(th))), int(np.rint(step * np.sin(th)))))
    return rows


def check_twin(device, tile, in_ch, cpad):
    shapes = SCENE_SHAPES(tile)
    scenes, labels, table = packed(shapes, in_ch, 5, device)
    n = len(shapes)
    rows = random_rows(shapes, tile, 100 + tile + in_ch)
    bad = [(n, 0, 0, 0, ONE, 0), (-1, ONE, ONE, 3, ONE, 0),          # no such scene
           (0, 0, 0, 0, 2 ** 20 + 1, 0), (0, 0, 0, 0, 0, -(2 ** 20) - 1),   # matrix out of range
           (0, 2 ** 46, 0, 0, ONE, 0), (0, 0, -(2 ** 46), 0, ONE, 0),       # centre out of range
           (2 ** 32, 0, 0, 0, ONE, 0), (0, 0, 0, 0, 2 ** 32 + ONE, 2 ** 32)]  # no 32-bit truncation
    wp = wrows(rows + bad, device)
    assert wp.shape[0] <= 150
    g = torch.Generator().manual_seed(tile)
    color = torch.stack([0.7 + 0.6 * torch.rand(wp.shape[0], generator=g),
                         0.3 * torch.rand(wp.shape[0], generator=g) - 0.15], 1).to(device)
    for col in (color, None):
        x, y = ops().warp_gather(scenes, labels, table, wp, col, tile, cpad)
        assert x.shape[-1] == cpad
        xr, yr = assert_batch_equals_twin(x, y, scenes, labels, table, wp, col, tile, in_ch)
        for i in range(len(rows), len(rows) + len(bad)):
            assert not x[i].any() and bool((y[i] == -100).all()), i
        assert bool((y[:len(rows)] >= 0).all())
    # the rows are resamplings, not permutations: values between the byte levels occur
    frac = (xr[:len(rows)] * 255.0) % 1.0
    assert float(((frac > 0.1) & (frac < 0.9)).float().mean()) > 0.3
    # a masked code equals its low three bits
    p6 = wrows([(2, 20 * ONE, 16 * ONE, 6, 50000, 23456)], device)
    x6, y6 = ops().warp_gather(scenes, labels, table, p6, None, tile, cpad)
    assert torch.equal(x6[0], x[5]) and torch.equal(y6[0], y[5])
    # a table row that does not lie inside the pixel buffer reads nothing
    wild = table.clone()
    wild[0, 0] = scenes.shape[0] - 1
    wild[1, 1] = -1
    xw, yw = ops().warp_gather(scenes, labels, wild, wrows([(0, 0, 0, 0, ONE, 0), (1, 0, 0, 0, ONE, 0)], device),
                               None, tile, cpad)
    assert not xw.any() and bool((yw == -100).all())
    empty = ops().warp_gather(scenes, labels, table, wp[:0], None, tile, cpad)
    assert empty[0].shape == (0, tile, tile, cpad) and empty[1].shape == (0, tile, tile)


def check_constant_image(device):
    """A constant image stays constant under any zoom, angle and overhang."""
    tile = 24
    table = torch.tensor([[0, 19, 31]], dtype=torch.int64, device=device)
    scenes = torch.tensor([37, 255, 0], dtype=torch.uint8, device=device).repeat(19 * 31, 1)
    labels = torch.full((19 * 31,), 4, dtype=torch.uint8, device=device)
    rows = [(0, cy, cx, code, A, Bm) for _, cy, cx, code, A, Bm in random_rows([(19, 31)], tile, 1, 40)]
    x, y = ops().warp_gather(scenes, labels, table, wrows(rows, device), None, tile, 8)
    want = (torch.tensor([37.0, 255.0, 0.0]) / 255.0).to(torch.bfloat16)
    assert torch.equal(x[..., :3].cpu(), want.expand(len(rows), tile, tile, 3)) and bool((y == 4).all())


# ------------------------------------------------------------------ 4. ramp (no twin involved)
def check_ramp(device):
    """On the image I(y, x) = (x, y) bilinear interpolation is exact (8 integer + 16 fraction
    bits fit a float32), so an interior crop's output is the coordinate itself."""
    H, W, tile = 64, 80, 24
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    scenes = torch.from_numpy(np.stack([xx, yy], -1).astype(np.uint8).reshape(-1, 2)).to(device)
    labels = torch.from_numpy(((7 * yy + 3 * xx) % 6).astype(np.uint8).reshape(-1)).to(device)
    table = torch.tensor([[0, H, W]], dtype=torch.int64, device=device)
    rows = [(0, 31 * ONE + 12345, 40 * ONE + 54321, 6, 50000, 23456),
            (0, 30 * ONE + 1, 38 * ONE + 65535, 0, -41234, 60000),
            (0, 32 * ONE, 41 * ONE + 32768, 5, 2 * ONE, 0),
            (0, 25 * ONE + 777, 45 * ONE + 31, 3, ONE // 4, -(ONE // 8))]
    x, y = ops().warp_gather(scenes, labels, table, wrows(rows, device), None, tile, 8)
    oy, ox = np.meshgrid(np.arange(tile, dtype=np.int64), np.arange(tile, dtype=np.int64), indexing="ij")
    for i, (_, cy, cx, code, A, Bm) in enumerate(rows):
        a, b = (ox, oy) if code & 4 else (oy, ox)
        a = tile - 1 - a if code & 2 else a
        b = tile - 1 - b if code & 1 else b
        v2, u2 = 2 * a - (tile - 1), 2 * b - (tile - 1)
        py = cy + ((Bm * u2 + A * v2) >> 1)
        px = cx + ((A * u2 - Bm * v2) >> 1)
        assert py.min() >= 0 and py.max() < (H - 1) * ONE and px.min() >= 0 and px.max() < (W - 1) * ONE
        want = np.stack([px, py], -1).astype(np.float32) * np.float32(2.0 ** -16) / np.float32(255.0)
        assert torch.equal(x[i, :, :, :2].cpu(), torch.from_numpy(want).to(torch.bfloat16)), i
        ry, rx = (py + 32768) >> 16, (px + 32768) >> 16
        assert np.array_equal(y[i].cpu().numpy(), (7 * ry + 3 * rx) % 6), i
    assert not x[..., 2:].any()


# ------------------------------------------------------------------ 5. warp_params
def check_params(device):
    from ddlpc.data.scenes import rotation_table, warp_params_reference, zoom_steps
    tile = 24
    shapes, table, cum = _params_setup(device, tile)
    steps = torch.from_numpy(zoom_steps(0.5, 2.0)).to(device)
    rot = torch.from_numpy(rotation_table(30.0)).to(device)
    assert steps.dtype == torch.int32 and steps.shape == (256,) and rot.dtype == torch.int32 and rot.shape == (256, 2)
    assert int(steps[0]) == int(np.rint(ONE / (0.5 * 4.0 ** (0.5 / 256)))) and ONE // 2 < int(steps[-1]) < int(steps[0]) < 2 * ONE
    assert int((steps.long() * steps.flip(0).long() - ONE * ONE).abs().max()) < 4 * ONE      # log-symmetric
    assert torch.equal(rot[:, 0], rot[:, 0].flip(0)) and torch.equal(rot[:, 1], -rot[:, 1].flip(0))
    assert int(rot[0, 1]) == int(np.rint(np.sin(np.deg2rad(-30 + 30 / 256)) * ONE))
    assert int((rot.long() ** 2).sum(1).sub(ONE * ONE).abs().max()) < 2 * ONE
    assert torch.equal(torch.from_numpy(rotation_table(0.0)), torch.tensor([[ONE, 0]], dtype=torch.int32).expand(256, 2))
    assert torch.equal(torch.from_numpy(zoom_steps(1.0, 1.0)), torch.full((256,), ONE, dtype=torch.int32))
    idx = torch.tensor(SAMPLES + list(range(100, 164)), dtype=torch.int64, device=device)
    F = ops()
    unit_s = torch.full((5,), ONE, dtype=torch.int32, device=device)
    unit_r = torch.tensor([[ONE, 0]] * 3, dtype=torch.int32, device=device)
    for mode in (0, 1, 2):
        for gj, bj in ((0.0, 0.0), (0.25, 0.125)):
            w, c = F.warp_params(idx, cum, table, steps, rot, 11, tile, mode, gj, bj)
            wr, cr = warp_params_reference(idx, cum, table, steps, rot, 11, tile, mode, gj, bj)
            assert w.dtype == torch.int64 and w.shape == (idx.numel(), 6)
            assert c.dtype == torch.float32 and c.shape == (idx.numel(), 2)
            assert torch.equal(w.cpu(), wr) and torch.equal(c.cpu(), cr), (mode, gj, bj)
            # scene, code and colour are crop_params's
            p, pc = F.crop_params(idx, cum, table, 11, tile, mode, gj, bj)
            assert torch.equal(w[:, 0], p[:, 0].long()) and torch.equal(w[:, 3], p[:, 3].long())
            assert torch.equal(c, pc)
            # (A, Bm) is a table step turned by at most 30 degrees
            for s, cy, cx, code, A, Bm in w.tolist():
                st = (A * A + Bm * Bm) ** 0.5
                assert int(steps.min()) - 2 <= st <= int(steps.max()) + 2 and abs(Bm) <= A * 0.5774 + 2
                assert 0 <= s < len(shapes) and 0 <= code <= (0, 3, 7)[mode]
            # without rotation A is the step: its footprint of F source pixels lies inside a
            # scene that holds it, and is centred on the origin-0 footprint in one that does not
            w0, _ = F.warp_params(idx, cum, table, steps, unit_r, 11, tile, mode, gj, bj)
            assert torch.equal(w0[:, [0, 3]], w[:, [0, 3]]) and not w0[:, 5].any()
            for s, cy, cx, code, A, Bm in w0.tolist():
                Fp = (tile * A + 65535) >> 16
                for cc_, n_ in ((cy, shapes[s][0]), (cx, shapes[s][1])):
                    assert (cc_ - (Fp - 1) * 32768) % ONE == 0
                    o = (cc_ - (Fp - 1) * 32768) // ONE
                    assert 0 <= o <= max(n_ - Fp, 0)
            # unit tables: the pair of ops is the crop pair
            w1, c1 = F.warp_params(idx, cum, table, unit_s, unit_r, 11, tile, mode, gj, bj)
            want = torch.stack([p[:, 0].long(), (2 * p[:, 1].long() + tile - 1) * 32768,
                                (2 * p[:, 2].long() + tile - 1) * 32768, p[:, 3].long(),
                                torch.full_like(p[:, 0], ONE).long(), torch.zeros_like(p[:, 0]).long()], 1)
            assert torch.equal(w1, want) and torch.equal(c1, pc)
    # ... end to end
    scenes, labels, _ = packed(shapes, 3, 8, device)
    w1, c1 = F.warp_params(idx, cum, table, unit_s, unit_r, 11, tile, 2, 0.25, 0.125)
    p, pc = F.crop_params(idx, cum, table, 11, tile, 2, 0.25, 0.125)
    xa, ya = F.warp_gather(scenes, labels, table, w1, c1, tile, 8)
    xb, yb = F.crop_gather(scenes, labels, table, p, pc, tile, 8)
    assert torch.equal(xa, xb) and torch.equal(ya, yb)
    # a row depends on (seed, sample number) only
    w, c = F.warp_params(idx, cum, table, steps, rot, 11, tile, 2, 0.25, 0.125)
    perm = torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(0)).to(device)
    wq, cq = F.warp_params(idx[perm], cum, table, steps, rot, 11, tile, 2, 0.25, 0.125)
    assert torch.equal(wq, w[perm]) and torch.equal(cq, c[perm])
    w2, _ = F.warp_params(idx, cum, table, steps, rot, 12, tile, 2, 0.25, 0.125)
    assert int((w2 != w).any(1).sum()) > idx.numel() // 2
    empty = F.warp_params(idx[:0], cum, table, steps, rot, 11, tile, 2, 0.0, 0.0)
    assert empty[0].shape == (0, 6) and empty[1].shape == (0, 2)
    # every table index occurs: the step index shows in A (rotation (ONE, 0)), the rotation
    # index in A with unit steps
    many = torch.arange(2 ** 16, dtype=torch.int64, device=device)
    s16 = (torch.arange(16, dtype=torch.int32, device=device) + 1) * 4096
    r1 = torch.tensor([[ONE, 0]], dtype=torch.int32, device=device)
    w, _ = F.warp_params(many, cum, table, s16, r1, 3, tile, 2, 0.0, 0.0)
    counts = torch.bincount((w[:, 4] // 4096 - 1).cpu(), minlength=16)
    assert counts.numel() == 16 and int(counts.min()) > 3500 and not w[:, 5].any()
    wr, _ = warp_params_reference(many[:4096], cum, table, s16, r1, 3, tile, 2)
    assert torch.equal(w[:4096].cpu(), wr)
    r16 = torch.stack([torch.arange(16) + 100, torch.arange(16) - 300], 1).to(torch.int32).to(device)
    w, _ = F.warp_params(many, cum, table, torch.tensor([ONE], dtype=torch.int32, device=device), r16, 3, tile, 2, 0.0, 0.0)
    counts = torch.bincount((w[:, 4] - 100).cpu(), minlength=16)
    assert counts.numel() == 16 and int(counts.min()) > 3500 and torch.equal(w[:, 5], w[:, 4] - 400)


# ------------------------------------------------------------------ 6. bad arguments
def check_rejects(device):
    scenes, labels, table = packed([(9, 9)], 3, 0, device)
    wp = wrows([(0, 4 * ONE, 4 * ONE, 0, ONE, 0)] * 2, device)
    F = ops()
    F.warp_gather(scenes, labels, table, wp, None, 4, 8)
    F.warp_gather(scenes, labels, table, wp, None, 4, 4)
    bad = [lambda: F.warp_gather(scenes.float(), labels, table, wp, None, 4, 8),
           lambda: F.warp_gather(scenes, labels[:-1], table, wp, None, 4, 8),
           lambda: F.warp_gather(scenes, labels, table.int(), wp, None, 4, 8),
           lambda: F.warp_gather(scenes, labels, table, wp.int(), None, 4, 8),
           lambda: F.warp_gather(scenes, labels, table, wp[:, :4].contiguous(), None, 4, 8),
           lambda: F.warp_gather(scenes, labels, table, wp, torch.ones(3, 2, device=device), 4, 8),
           lambda: F.warp_gather(scenes, labels, table, wp, torch.ones(2, 2, device=device).double(), 4, 8),
           lambda: F.warp_gather(scenes, labels, table, wp, None, 0, 8),
           lambda: F.warp_gather(scenes, labels, table, wp, None, 4, 3),
           lambda: F.warp_gather(scenes, labels, table, wp, None, 4, 16),
           lambda: F.warp_gather(torch.zeros(81, 5, dtype=torch.uint8, device=device), labels, table, wp, None, 4, 4),
           lambda: F.warp_gather(torch.zeros(81, 9, dtype=torch.uint8, device=device), labels, table, wp, None, 4, 8)]
    _, ptable, cum = _params_setup(device)
    idx = torch.arange(4, dtype=torch.int64, device=device)
    steps = torch.full((4,), ONE, dtype=torch.int32, device=device)
    rot = torch.tensor([[ONE, 0]] * 4, dtype=torch.int32, device=device)
    F.warp_params(idx, cum, ptable, steps, rot, 0, 24, 2, 0.0, 0.0)
    bad += [lambda: F.warp_params(idx.int(), cum, ptable, steps, rot, 0, 24, 2, 0.0, 0.0),
            lambda: F.warp_params(idx, cum[:-1].contiguous(), ptable, steps, rot, 0, 24, 2, 0.0, 0.0),
            lambda: F.warp_params(idx, cum, ptable, steps.long(), rot, 0, 24, 2, 0.0, 0.0),
            lambda: F.warp_params(idx, cum, ptable, steps, rot.long(), 0, 24, 2, 0.0, 0.0),
            lambda: F.warp_params(idx, cum, ptable, steps, rot.reshape(-1), 0, 24, 2, 0.0, 0.0),
            lambda: F.warp_params(idx, cum, ptable, steps[:0], rot, 0, 24, 2, 0.0, 0.0),
            lambda: F.warp_params(idx, cum, ptable, steps, rot[:0], 0, 24, 2, 0.0, 0.0),
            lambda: F.warp_params(idx, cum, ptable, steps.repeat(16385), rot, 0, 24, 2, 0.0, 0.0),
            lambda: F.warp_params(idx, cum, ptable, steps, rot, 0, 24, 3, 0.0, 0.0),
            lambda: F.warp_params(idx, cum, ptable, steps, rot, 0, 0, 2, 0.0, 0.0)]
    if torch.device(device).type != "cpu":                           # a tensor on the wrong device
        bad += [lambda: F.warp_gather(scenes, labels, table, wp.cpu(), None, 4, 8),
                lambda: F.warp_gather(scenes, labels.cpu(), table, wp, None, 4, 8),
                lambda: F.warp_gather(scenes, labels, table, wp, torch.ones(2, 2), 4, 8),
                lambda: F.warp_params(idx, cum, ptable, steps.cpu(), rot, 0, 24, 2, 0.0, 0.0),
                lambda: F.warp_params(idx, cum, ptable, steps, rot.cpu(), 0, 24, 2, 0.0, 0.0)]
    for i, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail(f"bad call {i} was accepted")
    from ddlpc.data.scenes import rotation_table, zoom_steps
    for fn in (lambda: zoom_steps(0.0, 1.0), lambda: zoom_steps(2.0, 1.0), lambda: zoom_steps(1.0, 2.0, 0),
               lambda: rotation_table(-1.0), lambda: rotation_table(10.0, 0)):
        with pytest.raises(ValueError):
            fn()


# ------------------------------------------------------------------ 7. the dataset
def check_dataset(device, tmp_path):
    from ddlpc.data import SceneCropDataset
    tile = 32
    d = str(tmp_path / "scenes")
    write_scenes(d)
    kw = dict(augment="d4", gain_jitter=0.2, bias_jitter=0.1, seed=4)
    warp = dict(zoom_min=0.5, zoom_max=2.0, rotate_deg=30.0)
    eng, eng_te = SceneCropDataset.from_dir(d, tile, 2, layout="engine", **kw, **warp)
    eng.to_device(device), eng_te.to_device(device)
    ref, _ = SceneCropDataset.from_dir(d, tile, 2, layout="nchw", **kw, **warp)
    assert eng.warped and ref.warped and not eng_te.warped          # the grid stays un-warped
    assert eng_te.steps is None and eng.steps.dtype == torch.int32 and eng.rot.shape == (256, 2)
    assert eng.steps.device.type == torch.device(device).type == eng.rot.device.type
    idx = [0, 5, 8, 3]
    p, c = eng.crop_rows(idx)
    assert p.dtype == torch.int64 and p.shape == (4, 6) and c.shape == (4, 2)
    assert p[:, 4].unique().numel() > 1 and bool((p[:, 5] != 0).any())
    x, y = eng.get(idx)
    xp = x._ddlpc_nhwc
    assert xp.shape == (4, tile, tile, 8) and xp.dtype == torch.bfloat16 and x.shape == (4, 3, tile, tile)
    assert xp.device.type == torch.device(device).type and y.dtype == torch.int64
    x2, y2 = eng.get(torch.tensor(idx, device=device))               # device indices, same batch
    assert torch.equal(x2._ddlpc_nhwc, xp) and torch.equal(y2, y)
    xn, yn = ref.get(idx)                                            # the numpy twins
    assert xn.dtype == torch.float32 and xn.shape == (4, 3, tile, tile)
    assert torch.equal(y.cpu(), yn) and torch.equal(x.cpu(), xn.to(torch.bfloat16))
    # a batch depends only on (seed, epoch * len + idx): other epochs, batch slots and splits
    eng.set_epoch(1), ref.set_epoch(1)
    x1, y1 = eng.get(idx)
    assert not torch.equal(x1._ddlpc_nhwc, xp)
    assert torch.equal(x1.cpu(), ref.get(idx)[0].to(torch.bfloat16))
    assert torch.equal(eng.sample_numbers([2]).cpu(), torch.tensor([len(eng) + 2]))
    eng.set_epoch(0)
    xs, ys = eng.get([3, 0])
    assert torch.equal(xs._ddlpc_nhwc, xp[[3, 0]]) and torch.equal(ys, y[[3, 0]])
    long_ = SceneCropDataset.from_dir(d, tile, 2, layout="engine", crops_per_epoch=2 * len(eng), **kw, **warp)[0]
    long_.to_device(device)
    xl, yl = long_.get([len(eng) + i for i in idx])                  # == epoch 1 of the short set
    assert torch.equal(xl._ddlpc_nhwc, x1._ddlpc_nhwc) and torch.equal(yl, y1)
    # a neutral data set is today's: the crop kernels, bit for bit
    for neutral in (dict(), dict(zoom_min=1.0, zoom_max=1.0, rotate_deg=0.0)):
        plain = SceneCropDataset.from_dir(d, tile, 2, layout="engine", **kw, **neutral)[0].to_device(device)
        assert not plain.warped and plain.steps is None and plain.rot is None
        pp, pc = plain.crop_rows(idx)
        want_p, want_c = ops().crop_params(plain.sample_numbers(idx), plain.cum, plain.table, 4, tile, 2, 0.2, 0.1)
        assert pp.dtype == torch.int32 and torch.equal(pp, want_p) and torch.equal(pc, want_c)
        xq, yq = plain.get(idx)
        xw, yw = ops().crop_gather(plain.pixels, plain.labels, plain.table, want_p, want_c, tile, 8)
        assert torch.equal(xq._ddlpc_nhwc, xw) and torch.equal(yq, yw)
        assert not torch.equal(xq._ddlpc_nhwc, xp)                   # ... and the warped set differs
    for one in (dict(zoom_min=0.5), dict(zoom_max=2.0), dict(rotate_deg=1.0)):
        assert SceneCropDataset.from_dir(d, tile, 2, **one)[0].warped
    with pytest.raises(IndexError):
        eng.get([len(eng)])


# ------------------------------------------------------------------ 8. config and CLI
def check_config_and_cli(tmp_path):
    import argparse
    import json
    from ddlpc.config import ModelConfig, TrainConfig, add_config_args, config_from_args
    d = TrainConfig().to_dict()
    assert (d["zoom_min"], d["zoom_max"], d["rotate_deg"]) == (1.0, 1.0, 0.0) and not TrainConfig().augmented
    c = TrainConfig(data="scene_dir", data_dir="/x", zoom_min=0.5, zoom_max=2.0, rotate_deg=30.0).validate()
    assert c.augmented
    assert TrainConfig.from_dict(json.loads(json.dumps(c.to_dict()))) == c
    ap = add_config_args(argparse.ArgumentParser())
    a = ap.parse_args(["--data", "scene_dir", "--data-dir", "/x", "--zoom-min", "0.5", "--zoom-max", "2",
                       "--rotate-deg", "30"])
    assert config_from_args(a) == c
    y = str(tmp_path / "c.yaml")
    with open(y, "w") as f:
        f.write("data: scene_dir\ndata_dir: /x\nzoom_min: 0.5\nzoom_max: 2.0\nrotate_deg: 30.0\n")
    assert TrainConfig.load(y) == c
    c3 = config_from_args(ap.parse_args(["--config", y, "--rotate-deg", "0"]))
    assert (c3.zoom_min, c3.zoom_max, c3.rotate_deg) == (0.5, 2.0, 0.0) and c3.augmented
    tiles = dict(data="vaihingen_dir", data_dir="/x")
    for bad in (dict(zoom_min=0.2), dict(zoom_max=4.5), dict(zoom_min=2.0, zoom_max=1.5), dict(zoom_max=0.5),
                dict(rotate_deg=-1.0), dict(rotate_deg=181.0)):
        with pytest.raises(ValueError):
            TrainConfig(**dict(tiles, **bad)).validate()
    for aug in (dict(zoom_min=0.5), dict(zoom_max=2.0), dict(rotate_deg=45.0), dict(zoom_min=0.25, zoom_max=4.0),
                dict(rotate_deg=180.0)):
        assert TrainConfig(**dict(tiles, **aug)).validate().augmented      # tiles go the scene path
        with pytest.raises(ValueError):                              # 2-D only
            TrainConfig(model=ModelConfig(dims=3), **dict(tiles, **aug)).validate()
        with pytest.raises(ValueError):                              # rendered tiles are not cropped
            TrainConfig(data="synthetic", **aug).validate()


# ------------------------------------------------------------------ 9. training
def check_training(device, tmp_path, model):
    """fit() on a directory of unequal scenes with zoom, rotation, D4 and colour jitter, and the
    batch stream across a resume: two epochs straight through == one epoch, checkpoint,
    resume, one epoch, bit for bit."""
    from ddlpc.data import SceneCropDataset
    from ddlpc.train.trainer import Trainer
    d = str(tmp_path / "scenes")
    write_training_scenes(d)
    warp = dict(zoom_min=0.5, zoom_max=2.0, rotate_deg=30.0, model=model)
    tr = Trainer(train_cfg(tmp_path / "full", d, **warp), device=device)
    assert isinstance(tr.train_set, SceneCropDataset) and tr.train_set.warped and len(tr.train_set) == 16
    assert isinstance(tr.test_set, SceneCropDataset) and not tr.test_set.warped
    x, _ = tr.train_set.get([0, 1])
    assert getattr(x, "_ddlpc_nhwc", None) is not None and x._ddlpc_nhwc.device.type == torch.device(device).type
    m = tr.fit()
    v = tr.validate()
    full = tr.flat.param_buf.clone()
    tr.close()
    assert m["steps"] == 8 and np.isfinite(m["loss"]) and np.isfinite(v["val_loss"])
    ck = str(tmp_path / "ck")
    t1 = Trainer(train_cfg(tmp_path / "p1", d, epochs=1, ckpt_dir=ck, log_dir=None, **warp), device=device)
    t1.fit()
    assert (t1.epoch, t1.step_count) == (1, 4)
    t1.close()
    t2 = Trainer(train_cfg(tmp_path / "p2", d, epochs=2, ckpt_dir=ck, resume="auto", log_dir=None, **warp),
                 device=device)
    assert t2.epoch == 1
    t2.fit()
    assert t2.step_count == 8 and t2.train_set.epoch == 1
    assert torch.equal(t2.flat.param_buf, full)
    t2.close()
