"""Whole-scene prediction: overlap-tile inference fused into the head.

The reference only dumps the arg-max of a few training tiles (ref.py:785-790) and the
trainer validates pre-cut, equal-sized tiles.  A real orthophoto (ISPRS Vaihingen: about
2500 x 2000 pixels) is predicted here with the U-Net paper's overlap-tile strategy:
overlapping windows, the image mirrored at its borders, the windows' class probabilities
blended.

* ``plan_windows`` cuts the scene into windows of ``tile`` pixels with stride
  ``s = tile - overlap``, in four colour groups (window row / column parity).  Two windows
  of one colour are at least ``2 s >= tile`` apart along some axis, so they never share a
  pixel: one launch blends a whole batch of them into the scene accumulator with plain
  read-modify-write — no float atomics, bit-reproducible results.
* ``blend_weights``: ``core`` (the original crop: every pixel from exactly one window) or
  ``cosine`` (raised-cosine ramps over the overlap; adjacent windows sum to 1).
* ``ScenePredictor`` uploads the scene once as uint8, cuts each batch of windows in the
  first conv's input layout (``window_gather``), runs the model in eval mode and blends:
  with the operator engine ``head_predict_accum`` computes the head, the softmax and the
  weighted accumulation from the last decoder block's pre-BatchNorm output in one kernel —
  the logits never reach HBM; without it (stock fp32 modules, ``fused=False``) the same
  result is composed from ``model(x)``, ``torch.softmax`` and slice-adds.
  ``scene_finalize`` turns the accumulator into the class map and the confusion matrix.
* Test-time augmentation (``tta="flip" | "d4"``): every window is predicted under 4 / 8
  symmetries of the square (the codes of ``crop_gather``, ``symmetry_maps``), the class
  probabilities are mapped back and averaged.  ``window_gather`` cuts the S views of a
  window and ``head_predict_accum`` un-maps, sums and blends them with ONE read-modify-write
  of the accumulator per window pixel.
* ``predict`` is the entry point behind ``python -m ddlpc predict``.
"""
from __future__ import annotations

import contextlib
import json
import math
import os
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

BLENDS = ("core", "cosine")
TTA_CODES = {"none": (0,), "flip": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


# ---------------------------------------------------------------------- plan and weights
def reflect(i: int, n: int) -> int:
    """Mirror index ``i`` into ``[0, n)`` without repeating the edge pixel (period
    ``2 (n - 1)``); the rule of the ``window_gather`` kernels."""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    i %= p
    return p - i if i >= n else i


def _check_plan(tile: int, overlap: int):
    if tile < 1:
        raise ValueError(f"tile must be positive, got {tile}")
    if overlap % 2 or not 0 <= overlap <= tile // 2:
        raise ValueError(f"overlap must be even and in [0, tile // 2], got {overlap} (tile {tile})")


def plan_windows(H: int, W: int, tile: int, overlap: int) -> List[List[Tuple[int, int]]]:
    """Window origins ``(y0, x0)`` as four colour groups (colour ``2 (i & 1) + (j & 1)`` of
    window row ``i`` / column ``j``, row-major inside a group).  Window ``(i, j)`` starts at
    ``(i s - m, j s - m)`` with ``s = tile - overlap``, ``m = overlap // 2``; its ``s x s``
    core (offset ``m``) tiles the scene exactly.  Origins may be negative and windows may
    overhang the scene."""
    _check_plan(tile, overlap)
    if H < 1 or W < 1:
        raise ValueError(f"empty scene {H} x {W}")
    s, m = tile - overlap, overlap // 2
    groups: List[List[Tuple[int, int]]] = [[], [], [], []]
    for i in range(-(-H // s)):
        for j in range(-(-W // s)):
            groups[2 * (i & 1) + (j & 1)].append((i * s - m, j * s - m))
    return groups


def blend_weights(tile: int, overlap: int, blend: str = "cosine") -> torch.Tensor:
    """Per-axis blend weights, fp32 ``[tile]`` (computed in fp64); the 2-D weight of a window
    pixel is the fp32 product ``w[y] * w[x]``."""
    _check_plan(tile, overlap)
    if blend not in BLENDS:
        raise ValueError(f"blend must be one of {BLENDS}, got {blend!r}")
    w = np.ones(tile, dtype=np.float64)
    m = overlap // 2
    if overlap and blend == "core":
        w[:m] = 0.0
        w[tile - m:] = 0.0
    elif overlap:
        r = 0.5 - 0.5 * np.cos(math.pi * (np.arange(overlap, dtype=np.float64) + 0.5) / overlap)
        w[:overlap] = r
        w[tile - overlap:] = r[::-1]
    return torch.from_numpy(w.astype(np.float32))


def symmetry_maps(tile: int, code: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Flat index maps of symmetry ``code`` (0..7, the convention of ``crop_gather``):
    network-side pixel ``(oy, ox)`` is window-frame pixel ``(a, b) = (oy, ox)``; ``code & 4``:
    swap ``a``, ``b``; ``code & 2``: ``a = tile - 1 - a``; ``code & 1``: ``b = tile - 1 - b``.
    -> ``(fwd, inv)``, int64 ``[tile * tile]``: ``view.flat[q] = window.flat[fwd[q]]`` and
    ``window.flat[n] = view.flat[inv[n]]``."""
    if not 0 <= code <= 7:
        raise ValueError(f"symmetry code must be in 0..7, got {code}")
    oy, ox = torch.meshgrid(torch.arange(tile), torch.arange(tile), indexing="ij")
    a, b = (ox, oy) if code & 4 else (oy, ox)
    if code & 2:
        a = tile - 1 - a
    if code & 1:
        b = tile - 1 - b
    fwd = (a * tile + b).reshape(-1)
    inv = torch.empty_like(fwd)
    inv[fwd] = torch.arange(tile * tile)
    return fwd, inv


def acc_channels(classes: int) -> int:
    """Channels of the scene accumulator: the classes and the weight sum, padded to whole
    float4s (a pixel is 16-byte aligned)."""
    return 4 * ((classes + 4) // 4)


# ---------------------------------------------------------------------- predictor
class ScenePredictor:
    """Overlap-tile prediction of whole scenes with a (2-D) ``UNet``.

    ``fused`` (default: whether the model has the operator engine attached) selects the
    one-kernel head + softmax + blend; ``fused=False`` is the unfused composition through
    ``model(x)`` (the test oracle, and the path of the stock modules).  ``autocast`` (an
    attribute, default off) runs the stock modules under bf16 autocast.

    ``tta`` (``"none"``, ``"flip"``: symmetry codes 0..3, ``"d4"``: codes 0..7) averages the
    class probabilities of every window over S symmetries.  ``window_batch`` stays the number
    of network inputs per forward: a pass takes ``max(1, window_batch // S)`` windows.
    ``windows`` counts the windows of the last scene, ``inputs`` its network inputs
    (``windows * S``)."""

    def __init__(self, model, tile: int, overlap: Optional[int] = None, blend: str = "cosine",
                 window_batch: int = 16, fused: Optional[bool] = None, tta: str = "none"):
        if getattr(model, "dims", 2) != 2:
            raise ValueError("scene prediction supports 2-D models only")
        overlap = (tile // 4) & ~1 if overlap is None else int(overlap)
        _check_plan(tile, overlap)
        if tile % (2 ** model.depth):
            raise ValueError(f"tile {tile} must be a multiple of 2**depth = {2 ** model.depth}")
        if window_batch < 1:
            raise ValueError("window_batch must be >= 1")
        if tta not in TTA_CODES:
            raise ValueError(f"tta must be one of {tuple(TTA_CODES)}, got {tta!r}")
        engine = getattr(model, "_engine", None)
        if fused is None:
            fused = engine is not None
        if fused and engine is None:
            raise ValueError("fused=True needs the operator engine (model.to_hip())")
        from .ops import _ext
        self.ops = _ext.ops()                      # fails loudly without the kernel library
        self.model = model
        self.tile, self.overlap, self.blend = int(tile), overlap, blend
        self.window_batch = int(window_batch)
        self.fused = bool(fused)
        self.autocast = False
        self.classes = int(model.conv_last.out_channels)
        self.in_channels = int(model.cfg.in_channels)
        self.win = blend_weights(tile, overlap, blend)
        self.tta = tta
        self.codes = TTA_CODES[tta]
        self.windows = 0                           # windows of the last scene
        self.inputs = 0                            # network inputs of the last scene
        self._codes: Dict[str, torch.Tensor] = {}
        self._maps: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._plans: Dict[Tuple[int, int, str], list] = {}

    @property
    def device(self) -> torch.device:
        return next(self.model.parameters()).device

    def _plan(self, H: int, W: int, dev: torch.device):
        key = (H, W, str(dev))
        if key not in self._plans:
            groups = plan_windows(H, W, self.tile, self.overlap)
            self._plans[key] = [(g, torch.tensor(g, dtype=torch.int32, device=dev).reshape(-1, 2))
                                for g in groups]
        return self._plans[key]

    def _scene(self, scene) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(scene)) if isinstance(scene, np.ndarray) else scene
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != self.in_channels:
            raise ValueError(f"scene must be uint8 [H, W, {self.in_channels}], got "
                             f"{t.dtype} {tuple(t.shape)}")
        return t.to(self.device).contiguous()

    @torch.no_grad()
    def accumulate(self, scene) -> torch.Tensor:
        """-> fp32 ``[H, W, KA]``: channels ``< K`` hold the weighted class probabilities,
        channel ``K`` the weight sum."""
        from .data.datasets import engine_input
        F = self.ops
        model, K = self.model, self.classes
        sc = self._scene(scene)
        dev = sc.device
        H, W = int(sc.shape[0]), int(sc.shape[1])
        win = self.win.to(dev)
        acc = torch.zeros(H, W, acc_channels(K), dtype=torch.float32, device=dev)
        w2 = (win[:, None] * win[None, :]) if not self.fused else None
        was_training = model.training
        model.eval()
        try:
            # a pass: ``per`` windows of one colour per forward, S views each (window-major)
            S = len(self.codes)
            per = max(1, self.window_batch // S)
            # (no codes tensor without augmentation: the ops then take code 0 with no host copy;
            # the unfused side always cuts plain windows)
            codes = self._codes_tensor(dev) if self.fused and self.tta != "none" else None
            self.windows = self.inputs = 0
            for host, origins in self._plan(H, W, dev):        # colour groups, in order
                for i in range(0, len(host), per):
                    o, ho = origins[i:i + per], host[i:i + per]
                    self.windows += int(o.shape[0])
                    self.inputs += int(o.shape[0]) * S
                    xw = F.window_gather(sc, o, self.tile, 8, codes)
                    if self.fused:
                        eng = model._engine
                        a, s = eng.features(engine_input(xw, self.in_channels), defer_last=True)
                        wh, bh = eng._head_params()
                        F.head_predict_accum(a, wh.detach().contiguous(), bh.detach().contiguous(),
                                             o, win, acc, s, codes)
                    elif self.tta == "none":
                        self._accumulate_unfused(engine_input(xw, self.in_channels), ho, w2, acc)
                    else:
                        self._accumulate_unfused_tta(xw, ho, w2, acc)
        finally:
            model.train(was_training)
        return acc

    def _codes_tensor(self, dev):
        key = str(dev)
        if key not in self._codes:
            self._codes[key] = torch.tensor(self.codes, dtype=torch.int32, device=dev)
        return self._codes[key]

    def _symmetry_maps(self, dev):
        key = str(dev)
        if key not in self._maps:
            maps = [symmetry_maps(self.tile, c) for c in self.codes]
            self._maps[key] = (torch.stack([m[0] for m in maps]).to(dev),
                               torch.stack([m[1] for m in maps]).to(dev))
        return self._maps[key]

    def _proba(self, x) -> torch.Tensor:
        model = self.model
        if model._engine is None:
            x = x.to(next(model.parameters()).dtype)
        ctx = (torch.autocast(x.device.type, dtype=torch.bfloat16) if self.autocast
               else contextlib.nullcontext())
        with ctx:
            logits = model(x)
        return torch.softmax(logits.float(), dim=1)

    def _accumulate_unfused(self, x, origins, w2, acc):
        self._slice_add(self._proba(x) * w2, origins, w2, acc)  # [B, K, t, t]

    def _accumulate_unfused_tta(self, xw, origins, w2, acc):
        """The plain windows ``xw`` under ``self.codes``: the views through the index maps, the
        probabilities mapped back and averaged."""
        from .data.datasets import engine_input
        t, S = self.tile, len(self.codes)
        B = int(xw.shape[0])
        fwd, inv = self._symmetry_maps(xw.device)
        xv = xw.reshape(B, t * t, 8)[:, fwd].reshape(B * S, t, t, 8)     # fwd [S, t * t]: window-major
        p = self._proba(engine_input(xv, self.in_channels))             # [B * S, K, t, t]
        p = p.reshape(B, S, self.classes, t * t)
        mean = p.gather(3, inv[None, :, None, :].expand_as(p)).sum(1) / S
        self._slice_add(mean.reshape(B, self.classes, t, t) * w2, origins, w2, acc)

    def _slice_add(self, p, origins, w2, acc):
        K, t = self.classes, self.tile
        H, W = acc.shape[0], acc.shape[1]
        for b, (y0, x0) in enumerate(origins):
            ys, xs = max(0, -y0), max(0, -x0)
            ye, xe = min(t, H - y0), min(t, W - x0)
            if ye <= ys or xe <= xs:
                continue
            dst = acc[y0 + ys:y0 + ye, x0 + xs:x0 + xe]
            dst[..., :K] += p[b, :, ys:ye, xs:xe].permute(1, 2, 0)
            dst[..., K] += w2[ys:ye, xs:xe]

    @torch.no_grad()
    def finalize(self, acc: torch.Tensor, labels=None, ignore_index: int = -100):
        """Accumulator -> (class map uint8 ``[H, W]`` on the host, confusion matrix int64
        ``[K, K]`` on the host — ``cm[label, pred]`` — or None without labels)."""
        lab = None
        if labels is not None:
            lab = torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) else labels
            if lab.dtype != torch.uint8 or tuple(lab.shape) != tuple(acc.shape[:2]):
                raise ValueError(f"labels must be uint8 {tuple(acc.shape[:2])}, got "
                                 f"{lab.dtype} {tuple(lab.shape)}")
            lab = lab.to(acc.device).contiguous()
        pred, cm = self.ops.scene_finalize(acc, self.classes, lab, ignore_index)
        return pred.cpu(), (cm.cpu() if lab is not None else None)

    def predict(self, scene, labels=None, ignore_index: int = -100):
        """-> (class map, confusion matrix or None): ``finalize(accumulate(scene), labels)``."""
        return self.finalize(self.accumulate(scene), labels, ignore_index)

    @torch.no_grad()
    def proba(self, scene) -> torch.Tensor:
        """-> blended class probabilities, fp32 ``[K, H, W]``."""
        return self.proba_of(self.accumulate(scene))

    def proba_of(self, acc: torch.Tensor) -> torch.Tensor:
        """Accumulator -> fp32 ``[K, H, W]``."""
        K = self.classes
        return (acc[..., :K] / acc[..., K:K + 1]).permute(2, 0, 1).contiguous()


# ---------------------------------------------------------------------- entry point
def metrics_of(cm: torch.Tensor) -> Dict[str, object]:
    """Pixel accuracy, per-class IoU and their mean over present classes from a confusion
    matrix ``cm[label, pred]`` (the formulas of ``Trainer.validate``)."""
    cmd = cm.double()
    inter = cmd.diag()
    union = cmd.sum(0) + cmd.sum(1) - inter
    iou = (inter / union.clamp_min(1)).tolist()
    present = [v for v, u in zip(iou, union.tolist()) if u > 0]
    return {"pixel_acc": float(inter.sum() / cmd.sum().clamp_min(1)), "iou": iou,
            "miou": sum(present) / max(len(present), 1)}


def list_scenes(inputs: str) -> Tuple[List[str], Optional[List[str]]]:
    """A file, or a directory in ``load_files``' convention: sorted names, a name containing
    ``.npy`` is a label map, anything else an image.  -> (images, labels or None)."""
    if not os.path.isdir(inputs):
        if not os.path.exists(inputs):
            raise FileNotFoundError(inputs)
        return [inputs], None
    images, labels = [], []
    for name in sorted(os.listdir(inputs)):
        (labels if ".npy" in name else images).append(os.path.join(inputs, name))
    if not images:
        raise ValueError(f"{inputs}: no images")
    if labels and len(labels) != len(images):
        raise ValueError(f"{inputs}: {len(images)} images but {len(labels)} label files")
    return images, (labels or None)


def predict(cfg, checkpoint: str, inputs: str, out_dir: str, device: Optional[str] = None,
            pred_tile: Optional[int] = None, overlap: Optional[int] = None, blend: str = "cosine",
            window_batch: int = 16, save_proba: bool = False, tta: str = "none") -> Dict[str, object]:
    """Predict every scene of ``inputs`` with the checkpoint's model.  Writes per scene
    ``<stem>.png`` (class indices), ``<stem>_color.png`` (Vaihingen palette, 6 classes) and
    optionally ``<stem>_proba.npy`` (fp16 ``[K, H, W]``), appends one line per scene to
    ``out_dir/predict.jsonl`` and returns the summary.  ``tta`` (``none``, ``flip``, ``d4``)
    averages every window over the symmetries of the square (test-time augmentation).  Under
    ``torchrun`` scenes are sharded ``i % world == rank``; only the confusion matrix (and the
    pixel count) is all-reduced."""
    import torch.distributed as dist
    from PIL import Image

    from .data.datasets import _PALETTE, _read_image
    from .models.unet import UNet
    from .ops import _ext
    from .parallel.dist import init_distributed
    from .train.checkpoint import load_checkpoint
    from .train.trainer import resolve_impl

    cfg.validate()
    if cfg.model.dims != 2:
        raise ValueError("predict supports 2-D models only")
    info = init_distributed(cfg.backend, cfg.timeout_s, device)
    dev = info.device
    model = UNet.from_config(cfg.model).to(dev)
    load_checkpoint(checkpoint, model, restore_rng=False)
    impl = resolve_impl(cfg.impl, dev, cfg.dtype)
    if impl == "hip":
        _ext.ops()                               # fail loudly if kernels are missing
        model.to_hip()
    elif dev.type == "cuda":
        model.to(memory_format=torch.channels_last)
    sp = ScenePredictor(model, pred_tile or cfg.tile, overlap, blend, window_batch, tta=tta)
    sp.autocast = dev.type == "cuda" and impl == "torch" and cfg.dtype == "bf16"
    K = sp.classes
    images, labels = list_scenes(inputs)
    os.makedirs(out_dir, exist_ok=True)
    total = torch.zeros(K * K + 1, dtype=torch.int64)
    palette = np.uint8(np.rint(_PALETTE * 255.0)) if K == 6 else None
    with open(os.path.join(out_dir, "predict.jsonl"), "a") as log:
        for i in range(info.rank, len(images), info.world_size):
            stem = os.path.splitext(os.path.basename(images[i]))[0]
            scene = _read_image(images[i])
            lab = np.load(labels[i]).astype("uint8") if labels is not None else None
            t0 = time.perf_counter()
            acc = sp.accumulate(scene)
            pred, cm = sp.finalize(acc, lab)
            ms = (time.perf_counter() - t0) * 1e3
            H, W = int(pred.shape[0]), int(pred.shape[1])
            rec = {"name": os.path.basename(images[i]), "H": H, "W": W, "windows": sp.windows,
                   "ms": ms, "tta": tta}
            if cm is not None:
                m = metrics_of(cm)
                rec.update(pixel_acc=m["pixel_acc"], iou=m["iou"])
                total[:K * K] += cm.reshape(-1)
            total[K * K] += H * W
            out = pred.numpy()
            Image.fromarray(out, mode="L").save(os.path.join(out_dir, stem + ".png"))
            if palette is not None:
                Image.fromarray(palette[out], mode="RGB").save(os.path.join(out_dir, stem + "_color.png"))
            if save_proba:
                np.save(os.path.join(out_dir, stem + "_proba.npy"),
                        sp.proba_of(acc).half().cpu().numpy())
            del acc
            log.write(json.dumps(rec) + "\n")
            log.flush()
    if dist.is_available() and dist.is_initialized():
        total = total.to(dev)
        dist.all_reduce(total)
        total = total.cpu()
    summary: Dict[str, object] = {"scenes": len(images), "pixels": int(total[K * K])}
    if labels is not None:
        summary.update(metrics_of(total[:K * K].reshape(K, K)))
    return summary
