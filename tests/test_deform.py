"""Elastic deformation of the device-cut crops: ``elastic_field`` / ``elastic_gather``
(``csrc/deform.hip``, CPU twins in ``csrc/cpu_ref.cpp``, recipe in ``csrc/data_math.h``) against
``warp_gather`` where the two must coincide and against the numpy twins of ``data/scenes.py``,
and their way into ``SceneCropDataset`` and the configuration.  Every comparison is bit for bit
(docs/TESTING.md, "Elastic deformation")."""
import argparse

import numpy as np
import pytest
import torch

from crop_cases import SCENE_SHAPES, ops, packed, write_scenes
from warp_cases import ONE, centre, random_rows, wrows
from ddlpc.config import TrainConfig, add_config_args, config_from_args
from ddlpc.data import (SceneCropDataset, elastic_amp, elastic_field_reference, elastic_gather_reference,
                        spline_table)

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
# (tile, grid, in_ch, cpad): tile 8 = one partial block, tile 40 = 2 x 2 ragged blocks whose
# border at 32 lies inside a spline cell; SCENE_SHAPES holds a 5 x 7 scene (the mirror wraps)
CASES = [(8, 1, 3, 8), (8, 3, 4, 8), (8, 16, 3, 8), (40, 1, 4, 8), (40, 3, 3, 8), (40, 16, 4, 8), (40, 3, 3, 4)]
gather_cases = pytest.mark.parametrize("tile,grid,in_ch,cpad", CASES)
devices = pytest.mark.parametrize("device", DEVICES)


def setup(device, tile, grid, in_ch):
    scenes, labels, table = packed(SCENE_SHAPES(tile), in_ch, 5, device)
    return scenes, labels, table, torch.from_numpy(spline_table(tile, grid)).to(device)


def colours(B, device):
    g = torch.Generator().manual_seed(B)
    return torch.stack([0.7 + 0.6 * torch.rand(B, generator=g), 0.3 * torch.rand(B, generator=g) - 0.15], 1).to(device)


def same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_spline_table_is_a_partition_of_unity():
    for tile, grid in [(t, g) for t, g, _, _ in CASES] + [(256, 3), (4096, 16), (7, 5)]:
        t = spline_table(tile, grid)
        a = np.arange(tile)
        assert t.dtype == np.int32 and t.shape == (tile, 5) and np.array_equal(t[:, 0], ((2 * a + 1) * grid) // (2 * tile))
        assert (t[:, 1:].sum(1) == 4096).all() and t[:, 1:].min() >= 0 and t[:, 1:].max() <= 2731
        u = ((2 * a + 1) * grid - 2 * tile * t[:, 0]) / (2 * tile)
        assert np.abs(t[:, 4] - 4096 * u ** 3 / 6).max() <= 2 and np.abs(t[:, 1] - 4096 * (1 - u) ** 3 / 6).max() <= 2


@devices
@gather_cases
def test_zero_lattice_equals_warp_gather(device, tile, grid, in_ch, cpad):
    scenes, labels, table, spline = setup(device, tile, grid, in_ch)
    wp = wrows(random_rows(SCENE_SHAPES(tile), tile, 11 + tile, 32), device)
    ctrl = torch.zeros(len(wp), grid + 3, grid + 3, 2, dtype=torch.int32, device=device)
    for col in (None, colours(len(wp), device)):
        got = ops().elastic_gather(scenes, labels, table, wp, col, ctrl, spline, tile, cpad)
        assert same(got, ops().warp_gather(scenes, labels, table, wp, col, tile, cpad))
    assert got[0].shape == (len(wp), tile, tile, cpad) and got[0].dtype == torch.bfloat16


@devices
@gather_cases
def test_constant_lattice_moves_the_centre(device, tile, grid, in_ch, cpad):
    scenes, labels, table, spline = setup(device, tile, grid, in_ch)
    shifts = [(256, -512), (-300, 77), (1, -1), (5000, 3333), (-70000, 131072), (-131072, 255), (0, 640), (129, 0)]
    rows = [(k, centre(3 * code - 5, tile), centre(2 - code, tile), code, ONE, 0) for code in range(8) for k in range(4)]
    d = torch.tensor([shifts[(i + i // 8) % 8] for i in range(len(rows))], dtype=torch.int64)
    moved = torch.tensor(rows, dtype=torch.int64)
    moved[:, 1:3] += d << 8
    ctrl = d.to(torch.int32).reshape(-1, 1, 1, 2).expand(-1, grid + 3, grid + 3, 2).contiguous().to(device)
    got = ops().elastic_gather(scenes, labels, table, wrows(rows, device), None, ctrl, spline, tile, cpad)
    assert same(got, ops().warp_gather(scenes, labels, table, moved.to(device), None, tile, cpad))


@devices
@gather_cases
def test_random_lattice_equals_numpy_twin(device, tile, grid, in_ch, cpad):
    scenes, labels, table, spline = setup(device, tile, grid, in_ch)
    n = table.shape[0]
    table = torch.cat([table, torch.tensor([[0, -1, 5]], device=device)])          # row n: not inside the buffer
    rows = random_rows(SCENE_SHAPES(tile), tile, 3 * tile + grid, 40)
    rows += [(n, 4 * ONE, 4 * ONE, 0, ONE, 0), (n + 1, ONE, ONE, 3, ONE, 0), (-1, 0, 0, 5, ONE, 0)]
    wp = wrows(rows, device)
    g = torch.Generator().manual_seed(tile + grid)
    ctrl = torch.randint(-20 * 256, 20 * 256, (len(rows), grid + 3, grid + 3, 2), generator=g, dtype=torch.int32)
    ctrl[0, 1, 2], ctrl[1, 0, 0] = torch.tensor([2 ** 17 + 9, -2 ** 31]), torch.tensor([2 ** 31 - 1, -2 ** 17 - 1])
    ctrl[2] = torch.tensor([2 ** 17, -2 ** 17])
    assert not torch.equal(ctrl[..., 0], ctrl[..., 1]) and not torch.equal(ctrl, ctrl.transpose(1, 2))
    for col in (colours(len(rows), device), None):
        x, y = ops().elastic_gather(scenes, labels, table, wp, col, ctrl.to(device), spline, tile, cpad)
        xr, yr = elastic_gather_reference(scenes, labels, table, wp, col, ctrl, spline, tile)
        assert torch.equal(y.cpu(), yr) and torch.equal(x[..., :in_ch].cpu(), xr.permute(0, 2, 3, 1).to(torch.bfloat16))
        assert not x[..., in_ch:].any() and not x[-3:].any() and bool((y[-3:] == -100).all()) and bool((y[:-3] >= 0).all())
    plain = ops().warp_gather(scenes, labels, table, wp, None, tile, cpad)
    assert float((y != plain[1]).float().mean()) > 0.2                              # the field moves pixels


@devices
@pytest.mark.parametrize("grid", [1, 3, 16])
def test_elastic_field(device, grid):
    amp = elastic_amp(10.0)
    assert amp == int(np.rint(10 * 65536 / np.sqrt(21845.0))) and elastic_amp(0.0) == 0
    idx = torch.cat([torch.tensor([0, 7, 2 ** 31 + 5, 2 ** 40 + 3]), torch.arange(100, 352)]).to(device)
    c = ops().elastic_field(idx, 11, amp, grid)
    assert c.dtype == torch.int32 and c.shape == (256, grid + 3, grid + 3, 2) and c.device.type == torch.device(device).type
    twin = elastic_field_reference(idx, 11, amp, grid)
    assert torch.equal(c.cpu(), twin)
    perm = torch.randperm(256, generator=torch.Generator().manual_seed(0)).to(device)
    assert torch.equal(ops().elastic_field(idx[perm], 11, amp, grid), c[perm])      # sample s, any batch slot
    assert not torch.equal(ops().elastic_field(idx, 12, amp, grid), c)
    assert not ops().elastic_field(idx, 11, 0, grid).any() and ops().elastic_field(idx[:0], 11, amp, grid).shape[0] == 0
    # 256 * 2 * (grid + 3)^2 >= 8192 draws: the sample deviation is within 5 % of sigma (the standard
    # error of a deviation estimated from 8192 draws is 0.8 %), the twin's on its own too
    for seed in (11, 12):
        t = elastic_field_reference(idx, seed, amp, grid).double() / 256
        assert abs(float(t.std()) / 10.0 - 1) < 0.05 and abs(float(t.mean())) < 1.0
    assert abs(float((c.double() / 256).std()) / 10.0 - 1) < 0.05


def bad_calls(device):
    scenes, labels, table, spline = setup(device, 8, 3, 3)
    wp = wrows([(0, 4 * ONE, 4 * ONE, 0, ONE, 0)] * 2, device)
    ctrl = torch.zeros(2, 6, 6, 2, dtype=torch.int32, device=device)
    idx = torch.arange(4, device=device)
    G, E = ops().elastic_gather, ops().elastic_field
    G(scenes, labels, table, wp, None, ctrl, spline, 8, 8), E(idx, 0, 5, 3)           # the good calls
    bad = {"ctrl_dtype": lambda: G(scenes, labels, table, wp, None, ctrl.long(), spline, 8, 8),
           "ctrl_batch": lambda: G(scenes, labels, table, wp, None, ctrl[:1], spline, 8, 8),
           "ctrl_not_square": lambda: G(scenes, labels, table, wp, None, ctrl[:, :5].contiguous(), spline, 8, 8),
           "ctrl_axes": lambda: G(scenes, labels, table, wp, None, ctrl[..., :1].contiguous(), spline, 8, 8),
           "grid_0": lambda: G(scenes, labels, table, wp, None, ctrl[:, :3, :3].contiguous(), spline, 8, 8),
           "grid_17": lambda: G(scenes, labels, table, wp, None, ctrl.new_zeros(2, 20, 20, 2), spline, 8, 8),
           "spline_dtype": lambda: G(scenes, labels, table, wp, None, ctrl, spline.long(), 8, 8),
           "spline_rows": lambda: G(scenes, labels, table, wp, None, ctrl, spline[:7], 8, 8),
           "spline_cols": lambda: G(scenes, labels, table, wp, None, ctrl, spline[:, :4].contiguous(), 8, 8),
           "tile_4097": lambda: G(scenes, labels, table, wp, None, ctrl, spline.new_zeros(4097, 5), 4097, 8),
           "wparams": lambda: G(scenes, labels, table, wp.int(), None, ctrl, spline, 8, 8),
           "cpad": lambda: G(scenes, labels, table, wp, None, ctrl, spline, 8, 3),
           "idx_dtype": lambda: E(idx.int(), 0, 5, 3), "field_grid_0": lambda: E(idx, 0, 5, 0),
           "field_grid_17": lambda: E(idx, 0, 5, 17), "amp_negative": lambda: E(idx, 0, -1, 3),
           "amp_large": lambda: E(idx, 0, 2 ** 20 + 1, 3)}
    if device != "cpu":
        bad.update(ctrl_device=lambda: G(scenes, labels, table, wp, None, ctrl.cpu(), spline, 8, 8),
                   spline_device=lambda: G(scenes, labels, table, wp, None, ctrl, spline.cpu(), 8, 8))
    return bad


BAD = ["ctrl_dtype", "ctrl_batch", "ctrl_not_square", "ctrl_axes", "grid_0", "grid_17", "spline_dtype", "spline_rows",
       "spline_cols", "tile_4097", "wparams", "cpad", "idx_dtype", "field_grid_0", "field_grid_17", "amp_negative",
       "amp_large", "ctrl_device", "spline_device"]


@devices
@pytest.mark.parametrize("name", BAD)
def test_bad_arguments_are_rejected(device, name):
    calls = bad_calls(device)
    assert set(calls) <= set(BAD)
    if name in calls:                                   # (a wrong-device tensor needs two devices)
        with pytest.raises(RuntimeError):
            calls[name]()


def test_config_and_cli():
    base = dict(data="scene_dir", data_dir="/x")
    c = TrainConfig(**base).validate()
    assert (c.elastic_sigma, c.elastic_grid) == (0.0, 3) and not c.augmented
    ap = add_config_args(argparse.ArgumentParser())
    c = config_from_args(ap.parse_args(["--data", "scene_dir", "--data-dir", "/x", "--elastic-sigma", "10", "--elastic-grid", "5"]))
    assert (c.elastic_sigma, c.elastic_grid) == (10.0, 5) and c.augmented and TrainConfig.from_dict(c.to_dict()) == c
    for bad in (dict(elastic_sigma=-1.0), dict(elastic_sigma=32.5), dict(elastic_grid=0), dict(elastic_grid=17),
                dict(elastic_sigma=1.0, tile=8192), dict(elastic_sigma=1.0, data="synthetic")):
        with pytest.raises(ValueError):
            TrainConfig(**dict(base, **bad)).validate()


@devices
def test_dataset(device, tmp_path):
    d = str(tmp_path / "scenes")
    write_scenes(d)
    kw = dict(augment="d4", gain_jitter=0.2, bias_jitter=0.1, seed=4)
    idx = [0, 5, 8, 3]
    for warp in (dict(), dict(zoom_min=0.5, zoom_max=2.0, rotate_deg=30.0)):
        make = lambda layout, **el: SceneCropDataset.from_dir(d, 32, 2, layout=layout, **kw, **warp, **el)  # noqa: E731
        eng, grid = make("engine", elastic_sigma=4.0)
        eng.to_device(device)
        assert eng.elastic and not grid.elastic and grid.spline is None and eng.spline.shape == (32, 5)
        x, y = eng.get(idx)
        xn, yn = make("nchw", elastic_sigma=4.0)[0].get(idx)                        # the numpy twins
        assert x._ddlpc_nhwc.shape == (4, 32, 32, 8) and torch.equal(y.cpu(), yn) and torch.equal(x.cpu(), xn.to(torch.bfloat16))
        again = make("engine", elastic_sigma=4.0)[0].to_device(device)             # the same (seed, epoch, idx)
        assert same(again.get(idx), (x, y)) and same(again.get([3, 0]), (x[[3, 0]], y[[3, 0]]))
        again.set_epoch(1)
        assert not torch.equal(again.get(idx)[0], x)
        plain, zero = make("engine")[0].to_device(device), make("engine", elastic_sigma=0.0, elastic_grid=7)[0].to_device(device)
        assert not zero.elastic and zero.spline is None and same(zero.get(idx), plain.get(idx))
        assert not torch.equal(plain.get(idx)[0], x)
