"""Training on whole scenes: augmented random crops cut on the device.

The reference trains on 127 pre-cut 512² tiles (ref.py:737) and serves them unchanged every
epoch.  The real ISPRS Vaihingen set is a few dozen scenes of roughly 2500 x 2000 pixels with
differing sizes; here they are trained on as they are:

* ``load_scenes`` reads a directory of images of any size with the pairing rule of
  ``load_files`` (sorted names, ``'.npy' in name`` = label map);
* ``SceneCropDataset`` packs the scenes into one uint8 pixel buffer ``[total_pixels, C]``, one
  uint8 label buffer and an int64 table of ``(pixel offset, H, W)`` rows, uploaded ONCE.  A
  batch is two operator calls: ``crop_params`` turns the batch's virtual sample numbers
  (``epoch * len + index``, formed on the device) into ``(scene, y0, x0, code)`` rows and a
  per-sample ``(gain, bias)`` — a counter-based hash, so a crop never depends on the rank,
  the batch slot or the resume point — and ``crop_gather`` cuts the tile x tile crops in the
  first conv's input layout, applying one of the 8 symmetries of the square (``code``) and
  the colour jitter on the way (``csrc/data.hip`` holds the recipe);
* the held-out scenes are served as a deterministic grid of un-augmented windows through
  the same ``crop_gather`` (``SceneCropDataset.test_grid``), so ``Trainer.validate()`` runs
  unchanged;
* a directory of pre-cut tiles is the same packing with one scene per tile
  (``SceneCropDataset.from_tiles``): a tile-sized scene always gets origin (0, 0).

* random zoom and rotation (``zoom_min`` / ``zoom_max`` / ``rotate_deg``): the crop is a
  resampled window — ``warp_params`` draws a zoom step and an angle from two integer tables
  built here (``zoom_steps``, ``rotation_table``) and ``warp_gather`` reads bilinear image
  taps and nearest labels at 16.16 fixed-point affine coordinates, in the same single pass.
  With zoom 1 and rotation 0 (the defaults) the crop kernels run, unchanged.

``crop_params_reference`` / ``crop_gather_reference`` and ``warp_params_reference`` /
``warp_gather_reference`` are the numpy twins of the kernels (the same bits); they serve
``layout="nchw"`` and are the oracle of the tests.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .datasets import TileDataset, _read_image, device_indices, engine_input

AUGMENT_MODES = ("none", "flip", "d4")
_M32 = np.uint64(0xFFFFFFFF)
_F = np.float32
ONE = 65536                              # 1.0 in the warp kernels' 16.16 fixed point
WARP_TABLE = 256                         # entries of the zoom and of the rotation table
WARP_MAX_COEF = 2 ** 20                  # warp_gather: |A|, |Bm| <= this (a step of 16 pixels)
WARP_MAX_CENTRE = 2 ** 46                # ... and |cy|, |cx| < this


# ---------------------------------------------------------------------- the numpy twins
def _mix32(x: np.ndarray) -> np.ndarray:
    """lowbias32 on uint64 arrays holding uint32 values (== csrc/data.hip mix32)."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def _reflect(i: np.ndarray, n: int) -> np.ndarray:
    """Mirror indices into [0, n): period 2 (n - 1), edge pixel not repeated."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = i % p                                        # numpy: the non-negative remainder
    return np.where(i >= n, p - i, i)


def origin_counts(table, tile: int) -> Tuple[np.ndarray, np.ndarray]:
    t = np.asarray(table, dtype=np.int64).reshape(-1, 3)
    return np.maximum(t[:, 1] - tile, 0) + 1, np.maximum(t[:, 2] - tile, 0) + 1


def crop_cum(table, tile: int) -> np.ndarray:
    """int64 [n + 1]: prefix sum of the scenes' valid-origin counts (the sampling weights)."""
    ny, nx = origin_counts(table, tile)
    cum = np.concatenate([[0], np.cumsum(ny * nx)]).astype(np.int64)
    if len(cum) < 2:
        raise ValueError("no scenes")
    if int(cum[-1]) >= 2 ** 32:
        raise ValueError(f"{int(cum[-1])} valid crop origins: the sampler draws from < 2^32")
    return cum


def crop_params_reference(idx, cum, table, seed: int, tile: int, mode: int,
                          gain_jitter: float = 0.0, bias_jitter: float = 0.0
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """numpy twin of the ``crop_params`` kernels: params int32 [B, 4], color fp32 [B, 2]."""
    s = np.asarray(torch.as_tensor(idx, dtype=torch.int64).reshape(-1).cpu().numpy()).astype(np.uint64)
    cum = np.asarray(torch.as_tensor(cum).cpu().numpy(), dtype=np.int64)
    table = np.asarray(torch.as_tensor(table).cpu().numpy(), dtype=np.int64).reshape(-1, 3)
    skey = _mix32(np.array([(seed & 0xFFFFFFFF) ^ 0xC2B2AE35], dtype=np.uint64))
    hi = _mix32(((s >> np.uint64(32)) + np.uint64(0x85EBCA6B)) & _M32)
    key = _mix32(_mix32(skey ^ (s & _M32)) ^ hi)
    r = [_mix32((key + np.uint64(((j + 1) * 0x9E3779B9) & 0xFFFFFFFF)) & _M32) for j in range(6)]
    t = (r[0] * np.uint64(int(cum[-1]))) >> np.uint64(32)            # < 2^64: cum[n] < 2^32
    sc = np.searchsorted(cum.astype(np.uint64), t, side="right").astype(np.int64) - 1
    ny, nx = origin_counts(table, tile)
    y0 = (r[1] * ny[sc].astype(np.uint64)) >> np.uint64(32)
    x0 = (r[2] * nx[sc].astype(np.uint64)) >> np.uint64(32)
    code = (r[3] & np.uint64((0, 3, 7)[mode])).astype(np.int64)
    params = np.stack([sc, y0.astype(np.int64), x0.astype(np.int64), code], 1).astype(np.int32)

    def centred(h):                                   # 2 u24(h) - 1, each op rounded in fp32
        u = (h >> np.uint64(8)).astype(_F) * _F(1.0 / 16777216.0)
        return _F(2.0) * u + _F(-1.0)
    gain = _F(1.0) + _F(gain_jitter) * centred(r[4])
    bias = _F(bias_jitter) * centred(r[5])
    color = np.stack([gain, bias], 1).astype(_F)
    return torch.from_numpy(params), torch.from_numpy(color)


def crop_gather_reference(scenes, labels, table, params, color, tile: int
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """numpy twin of the ``crop_gather`` kernels: float32 NCHW (before the bf16 rounding) and
    int64 labels.  The crop is cut out with mirrored indices, then ``[::-1]`` for code bit 2,
    ``[:, ::-1]`` for bit 1, ``swapaxes(0, 1)`` for bit 4."""
    scenes = torch.as_tensor(scenes).cpu().numpy()
    labels = torch.as_tensor(labels).cpu().numpy()
    table = torch.as_tensor(table).cpu().numpy().reshape(-1, 3)
    params = torch.as_tensor(params).cpu().numpy()
    col = None if color is None else torch.as_tensor(color).cpu().numpy().astype(_F)
    B, C, n = params.shape[0], scenes.shape[1], table.shape[0]
    x = np.zeros((B, tile, tile, C), dtype=_F)
    y = np.full((B, tile, tile), -100, dtype=np.int64)
    ar = np.arange(tile, dtype=np.int64)
    for b in range(B):
        s, y0, x0, code = (int(v) for v in params[b])
        if not 0 <= s < n:
            continue                                  # reads nothing: zero image, ignored labels
        off, H, W = (int(v) for v in table[s])
        iy, ix = _reflect(y0 + ar, H), _reflect(x0 + ar, W)
        img = scenes[off:off + H * W].reshape(H, W, C)[iy][:, ix]
        lab = labels[off:off + H * W].reshape(H, W)[iy][:, ix]
        if code & 2:
            img, lab = img[::-1], lab[::-1]
        if code & 1:
            img, lab = img[:, ::-1], lab[:, ::-1]
        if code & 4:
            img, lab = img.swapaxes(0, 1), lab.swapaxes(0, 1)
        v = img.astype(_F) / _F(255.0)
        if col is not None:
            v = np.clip(v * col[b, 0] + col[b, 1], _F(0.0), _F(1.0))
        x[b], y[b] = v, lab
    return torch.from_numpy(x).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(y)


# ---------------------------------------------------------------------- warped crops
# Random zoom and rotation (the recipe: csrc/data.hip).  Coordinates are 16.16 fixed point in
# int64; the zoom and the angle reach the kernels only as integer tables built here, in
# float64, once per data set — there is no device pow / cos to match.
def zoom_steps(zoom_min: float, zoom_max: float, S: int = WARP_TABLE) -> np.ndarray:
    """int32 [S]: source pixels per output pixel in 16.16, ``rint(ONE / z_k)`` for the
    log-uniform zooms ``z_k = zoom_min * (zoom_max / zoom_min) ** ((k + 0.5) / S)``."""
    if not (0.0 < zoom_min <= zoom_max) or S < 1:
        raise ValueError("zoom_steps needs 0 < zoom_min <= zoom_max and S >= 1")
    k = (np.arange(S, dtype=np.float64) + 0.5) / S
    z = np.float64(zoom_min) * np.power(np.float64(zoom_max) / np.float64(zoom_min), k)
    return np.rint(ONE / z).astype(np.int32)


def rotation_table(rotate_deg: float, T: int = WARP_TABLE) -> np.ndarray:
    """int32 [T, 2]: ``(rint(cos t_k * ONE), rint(sin t_k * ONE))`` for the angles
    ``t_k = -rotate_deg + (k + 0.5) * 2 rotate_deg / T``; all ``(ONE, 0)`` for 0 degrees."""
    if rotate_deg < 0.0 or T < 1:
        raise ValueError("rotation_table needs rotate_deg >= 0 and T >= 1")
    t = np.deg2rad(-np.float64(rotate_deg) + (np.arange(T, dtype=np.float64) + 0.5) * 2.0 * rotate_deg / T)
    return np.stack([np.rint(np.cos(t) * ONE), np.rint(np.sin(t) * ONE)], 1).astype(np.int32)


def _footprint_centre(r: np.ndarray, size: np.ndarray, F: np.ndarray) -> np.ndarray:
    """Centre (16.16) of an F-pixel footprint whose origin is drawn from ``max(size - F, 0) +
    1`` positions: ``(2 origin + F - 1) * 32768``."""
    n = (np.maximum(size - F, 0) + 1).astype(np.uint64)
    o = ((r * n) >> np.uint64(32)).astype(np.int64)
    return (2 * o + F - 1) * 32768


def warp_params_reference(idx, cum, table, steps, rot, seed: int, tile: int, mode: int,
                          gain_jitter: float = 0.0, bias_jitter: float = 0.0
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """numpy twin of the ``warp_params`` kernels: wparams int64 [B, 6] of ``(scene, cy, cx,
    code, A, Bm)`` rows, color fp32 [B, 2].  Scene, code and colour are ``crop_params``'s."""
    p, color = crop_params_reference(idx, cum, table, seed, tile, mode, gain_jitter, bias_jitter)
    s = np.asarray(torch.as_tensor(idx, dtype=torch.int64).reshape(-1).cpu().numpy()).astype(np.uint64)
    table = np.asarray(torch.as_tensor(table).cpu().numpy(), dtype=np.int64).reshape(-1, 3)
    steps = np.asarray(torch.as_tensor(steps).cpu().numpy(), dtype=np.int64).reshape(-1)
    rot = np.asarray(torch.as_tensor(rot).cpu().numpy(), dtype=np.int64).reshape(-1, 2)
    skey = _mix32(np.array([(seed & 0xFFFFFFFF) ^ 0xC2B2AE35], dtype=np.uint64))
    hi = _mix32(((s >> np.uint64(32)) + np.uint64(0x85EBCA6B)) & _M32)
    key = _mix32(_mix32(skey ^ (s & _M32)) ^ hi)
    r = {j: _mix32((key + np.uint64(((j + 1) * 0x9E3779B9) & 0xFFFFFFFF)) & _M32) for j in (1, 2, 6, 7)}
    sc = p[:, 0].numpy().astype(np.int64)
    code = p[:, 3].numpy().astype(np.int64)
    step = steps[((r[6] * np.uint64(len(steps))) >> np.uint64(32)).astype(np.int64)]
    cs = rot[((r[7] * np.uint64(len(rot))) >> np.uint64(32)).astype(np.int64)]
    A = (step * cs[:, 0] + 32768) >> 16
    Bm = (step * cs[:, 1] + 32768) >> 16
    F = (tile * step + 65535) >> 16
    cy = _footprint_centre(r[1], table[sc, 1], F)
    cx = _footprint_centre(r[2], table[sc, 2], F)
    return torch.from_numpy(np.stack([sc, cy, cx, code, A, Bm], 1).astype(np.int64)), color


def warp_gather_reference(scenes, labels, table, wparams, color, tile: int
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """numpy twin of the ``warp_gather`` kernels: float32 NCHW (before the bf16 rounding) and
    int64 labels.  Bilinear image taps and nearest labels at the affine coordinates of
    csrc/data.hip; every float32 operation rounds on its own."""
    scenes = torch.as_tensor(scenes).cpu().numpy()
    labels = torch.as_tensor(labels).cpu().numpy()
    table = torch.as_tensor(table).cpu().numpy().reshape(-1, 3)
    wp = torch.as_tensor(wparams).cpu().numpy().astype(np.int64)
    col = None if color is None else torch.as_tensor(color).cpu().numpy().astype(_F)
    B, C, n, P = wp.shape[0], scenes.shape[1], table.shape[0], labels.shape[0]
    x = np.zeros((B, tile, tile, C), dtype=_F)
    y = np.full((B, tile, tile), -100, dtype=np.int64)
    oy, ox = np.meshgrid(np.arange(tile, dtype=np.int64), np.arange(tile, dtype=np.int64), indexing="ij")
    for b in range(B):
        s, cy, cx, code, A, Bm = (int(v) for v in wp[b])
        code &= 7
        if not 0 <= s < n or max(abs(A), abs(Bm)) > WARP_MAX_COEF or max(abs(cy), abs(cx)) >= WARP_MAX_CENTRE:
            continue                                  # reads nothing: zero image, ignored labels
        off, H, W = (int(v) for v in table[s])
        if not (1 <= H < 2 ** 30 and 1 <= W < 2 ** 30 and 0 <= off <= P and H * W <= P - off):
            continue
        a, c = (ox, oy) if code & 4 else (oy, ox)
        if code & 2:
            a = tile - 1 - a
        if code & 1:
            c = tile - 1 - c
        v2, u2 = 2 * a - (tile - 1), 2 * c - (tile - 1)
        py = cy + ((Bm * u2 + A * v2) >> 1)
        px = cx + ((A * u2 - Bm * v2) >> 1)
        iy, ix = py >> 16, px >> 16
        wy = (py & 65535).astype(_F) * _F(2.0 ** -16)
        wx = (px & 65535).astype(_F) * _F(2.0 ** -16)
        img = scenes[off:off + H * W].reshape(H, W, C)
        r0, r1 = _reflect(iy, H), _reflect(iy + 1, H)
        c0, c1 = _reflect(ix, W), _reflect(ix + 1, W)
        p00, p01 = img[r0, c0].astype(_F), img[r0, c1].astype(_F)
        p10, p11 = img[r1, c0].astype(_F), img[r1, c1].astype(_F)
        top = p00 + (p01 - p00) * wx[..., None]
        bot = p10 + (p11 - p10) * wx[..., None]
        v = (top + (bot - top) * wy[..., None]) / _F(255.0)
        if col is not None:
            v = np.clip(v * col[b, 0] + col[b, 1], _F(0.0), _F(1.0))
        x[b] = v
        y[b] = labels[off:off + H * W].reshape(H, W)[_reflect((py + 32768) >> 16, H),
                                                     _reflect((px + 32768) >> 16, W)]
    return torch.from_numpy(x).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(y)


# ---------------------------------------------------------------------- directory loader
Scene = Tuple[np.ndarray, np.ndarray]


def load_scenes(path: str, test_holdout: int = 30) -> Tuple[List[Scene], List[Scene]]:
    """``load_files`` for images of differing sizes: the same sorted image / ``.npy`` label
    pairing, every label map checked against its image; the last ``test_holdout`` scenes are
    held out.  Returns ``(train, test)`` lists of ``(uint8 HWC image, uint8 HW labels)``."""
    xs, ys, names = [], [], []
    for name in sorted(os.listdir(path)):
        full = os.path.join(path, name)
        if ".npy" in name:
            ys.append(np.load(full))
        else:
            xs.append(_read_image(full))
            names.append(name)
    if len(xs) != len(ys):
        raise ValueError(f"{path}: {len(xs)} images but {len(ys)} label files")
    out = []
    for name, x, y in zip(names, xs, ys):
        x = np.asarray(x)
        if x.ndim == 2:
            x = x[:, :, None]
        if x.dtype != np.uint8 or x.ndim != 3:
            raise TypeError(f"{path}/{name}: scenes are uint8 H x W x C images")
        if tuple(y.shape) != tuple(x.shape[:2]):
            raise ValueError(f"{path}/{name}: label map {tuple(y.shape)} does not match the image "
                             f"{tuple(x.shape[:2])}")
        out.append((x, np.asarray(y).astype(np.uint8)))
    if len({s[0].shape[2] for s in out}) > 1:
        raise ValueError(f"{path}: scenes differ in channel count")
    if test_holdout > 0:
        return out[:-test_holdout], out[-test_holdout:]
    return out, []


def grid_origins(H: int, W: int, tile: int) -> List[Tuple[int, int]]:
    """Origins of the evaluation windows of one scene: stride ``tile``, the last window of
    each direction aligned to the scene's end; a scene smaller than the tile is one window
    at 0 (mirrored)."""
    def axis(n):
        if n <= tile:
            return [0]
        o = list(range(0, n - tile, tile))
        return o + [n - tile]
    return [(y, x) for y in axis(H) for x in axis(W)]


# ---------------------------------------------------------------------- the dataset
class SceneCropDataset:
    """Packed scenes served as tile x tile crops (see the module docstring).

    Two modes: random augmented crops (``params=None``; ``len`` = ``crops_per_epoch``, sample
    ``i`` of epoch ``e`` is virtual sample ``e * len + i``), or an explicit list of
    ``(scene, y0, x0, code)`` rows (``params``; the evaluation grid), un-jittered.
    ``layout="engine"`` calls the ``crop_params`` / ``crop_gather`` operators (the gfx950
    kernels on a GPU, their C++ twins on the CPU); ``layout="nchw"`` the numpy twins
    (float32 NCHW, host)."""

    def __init__(self, scenes: Sequence[Scene], tile: int, crops_per_epoch: int = 0,
                 augment: str = "none", gain_jitter: float = 0.0, bias_jitter: float = 0.0,
                 seed: int = 0, layout: str = "nchw", params=None, zoom_min: float = 1.0,
                 zoom_max: float = 1.0, rotate_deg: float = 0.0):
        if augment not in AUGMENT_MODES:
            raise ValueError(f"augment={augment!r} not in {AUGMENT_MODES}")
        if layout not in ("nchw", "engine"):
            raise ValueError(f"layout={layout!r}")
        if tile < 1 or not scenes:
            raise ValueError("SceneCropDataset needs tile >= 1 and at least one scene")
        self.tile, self.seed, self.layout = int(tile), int(seed), layout
        self.mode = AUGMENT_MODES.index(augment)
        self.gain_jitter, self.bias_jitter = float(gain_jitter), float(bias_jitter)
        self.zoom_min, self.zoom_max, self.rotate_deg = float(zoom_min), float(zoom_max), float(rotate_deg)
        rows, off = [], 0
        for x, y in scenes:
            if x.dtype != np.uint8 or x.ndim != 3 or tuple(y.shape) != tuple(x.shape[:2]):
                raise ValueError("scenes are (uint8 H x W x C image, H x W label map) pairs")
            rows.append((off, x.shape[0], x.shape[1]))
            off += x.shape[0] * x.shape[1]
        self.in_channels = int(scenes[0][0].shape[2])
        if self.in_channels > 8:
            raise ValueError("at most 8 input channels")
        self.pixels = torch.from_numpy(np.concatenate(
            [np.ascontiguousarray(x).reshape(-1, self.in_channels) for x, _ in scenes]))
        self.labels = torch.from_numpy(np.concatenate(
            [np.ascontiguousarray(y, dtype=np.uint8).reshape(-1) for _, y in scenes]))
        self.table = torch.tensor(rows, dtype=torch.int64)
        self.cum = torch.from_numpy(crop_cum(self.table.numpy(), self.tile))
        self.params = None if params is None else \
            torch.as_tensor(params, dtype=torch.int32).reshape(-1, 4).contiguous()
        # random zoom / rotation: the integer tables of warp_params (None = the crop kernels)
        self.steps = self.rot = None
        if self.warped:
            self.steps = torch.from_numpy(zoom_steps(self.zoom_min, self.zoom_max))
            self.rot = torch.from_numpy(rotation_table(self.rotate_deg))
        t2 = self.tile * self.tile
        self.length = len(self.params) if self.params is not None else \
            int(crops_per_epoch) if crops_per_epoch > 0 else -(-off // t2)
        self.epoch = 0
        self.device = torch.device("cpu")

    # ---- constructors
    @classmethod
    def from_dir(cls, path: str, tile: int, test_holdout: int = 30, **kw):
        """``(train, test)``: random crops of the training scenes, the window grid of the
        held-out ones (``None`` without a hold-out)."""
        tr, te = load_scenes(path, test_holdout)
        if not tr:
            raise ValueError(f"{path}: no training scenes left after holding out {test_holdout}")
        return cls(tr, tile, **kw), (cls.test_grid(te, tile, kw.get("layout", "nchw")) if te else None)

    @classmethod
    def test_grid(cls, scenes: Sequence[Scene], tile: int, layout: str = "nchw"):
        rows = [(k, y0, x0, 0) for k, (x, _) in enumerate(scenes)
                for y0, x0 in grid_origins(x.shape[0], x.shape[1], tile)]
        return cls(scenes, tile, layout=layout, params=rows)

    @classmethod
    def from_tiles(cls, tiles: TileDataset, tile: int, **kw):
        """A pre-cut tile set as one scene per tile (``params=...`` for the plain tiles)."""
        if tiles.x.dim() != 4:
            raise ValueError("augmented crops are 2-D")
        x, y = tiles.x.numpy(), tiles.y.numpy()
        return cls([(x[i], y[i]) for i in range(len(x))], tile, **kw)

    # ---- placement
    def to_device(self, device, layout: Optional[str] = None, budget_bytes: Optional[int] = None):
        """Upload the packed scenes (once).  The set must be resident: above the HBM budget
        (default: half the free memory) this raises — host-streamed scene sets are not built."""
        device = torch.device(device)
        if layout is not None:
            self.layout = layout
        if self.layout == "nchw":
            return self                    # the numpy twins cut on the host; batches are copied
        nbytes = self.pixels.numel() + self.labels.numel()
        if device.type == "cuda":
            if budget_bytes is None:
                free, _ = torch.cuda.mem_get_info(device)
                budget_bytes = free // 2
            if nbytes > budget_bytes:
                raise MemoryError(f"scene set of {nbytes} bytes exceeds the HBM budget of "
                                  f"{budget_bytes} bytes; scene sets are served from HBM only "
                                  f"(raise data_hbm_gb or train on fewer scenes)")
        for name in ("pixels", "labels", "table", "cum", "params", "steps", "rot"):
            t = getattr(self, name)
            if t is not None:
                setattr(self, name, t.to(device))
        self.device = device
        return self

    @property
    def resident(self) -> bool:
        return True

    @property
    def warped(self) -> bool:
        """Random crops are zoomed / rotated: batches go through ``warp_params`` / ``warp_gather``
        (an explicit ``params`` list, the evaluation grid, stays un-warped)."""
        return self.params is None and (self.zoom_min != 1.0 or self.zoom_max != 1.0 or
                                        self.rotate_deg != 0.0)

    def __len__(self):
        return self.length

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    # ---- batches
    def sample_numbers(self, idx) -> torch.Tensor:
        """Virtual sample numbers ``epoch * len + idx`` on the data's device (no host sync)."""
        return device_indices(idx, self.device) + self.epoch * self.length

    def crop_rows(self, idx):
        """``(params, color)`` of a batch: the rows ``crop_gather`` is called with."""
        if not torch.is_tensor(idx) or idx.device.type == "cpu":
            ii = torch.as_tensor(idx, dtype=torch.int64).reshape(-1)
            if ii.numel() and (int(ii.min()) < 0 or int(ii.max()) >= len(self)):
                raise IndexError(f"sample index out of range [0, {len(self)})")
        if self.params is not None:
            return self.params.index_select(0, device_indices(idx, self.device)), None
        s = self.sample_numbers(idx)
        jitter = (self.seed, self.tile, self.mode, self.gain_jitter, self.bias_jitter)
        if self.warped and self.layout == "engine":
            from ..ops import _ext
            p, c = _ext.ops().warp_params(s, self.cum, self.table, self.steps, self.rot, *jitter)
        elif self.warped:
            p, c = warp_params_reference(s, self.cum, self.table, self.steps, self.rot, *jitter)
        elif self.layout == "engine":
            from ..ops import _ext
            p, c = _ext.ops().crop_params(s, self.cum, self.table, self.seed, self.tile, self.mode,
                                          self.gain_jitter, self.bias_jitter)
        else:
            p, c = crop_params_reference(s, self.cum, self.table, self.seed, self.tile, self.mode,
                                         self.gain_jitter, self.bias_jitter)
        return p, (c if (self.gain_jitter or self.bias_jitter) else None)

    def get(self, idx) -> Tuple[torch.Tensor, torch.Tensor]:
        p, c = self.crop_rows(idx)
        if self.layout == "engine":
            from ..ops import _ext
            gather = _ext.ops().warp_gather if self.warped else _ext.ops().crop_gather
            xp, y = gather(self.pixels, self.labels, self.table, p, c, self.tile, 8)
            return engine_input(xp, self.in_channels), y
        if self.warped:
            return warp_gather_reference(self.pixels, self.labels, self.table, p, c, self.tile)
        return crop_gather_reference(self.pixels, self.labels, self.table, p, c, self.tile)
