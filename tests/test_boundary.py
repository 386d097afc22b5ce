"""``label_dist2`` / ``label_erode`` (``csrc/boundary.hip``, CPU twin in ``csrc/cpu_ref.cpp``) and
their way into ``Trainer`` and ``ScenePredictor``, against a torch brute force over all 33 x 33
offsets in integers on the CPU: exact equality throughout (docs/TESTING.md, "Label boundaries")."""
import argparse

import pytest
import torch
import torch.nn.functional as F

import predict_cases as pc
from ddlpc.config import ModelConfig, TrainConfig, add_config_args, config_from_args
from ddlpc.data import device_random_batch
from ddlpc.infer import ScenePredictor, metrics_of
from ddlpc.ops import _ext, boundary
from ddlpc.train.trainer import Trainer

GPU = pytest.param("cuda", marks=pytest.mark.gpu)


def brute_d2(lab, K, ignore):
    l = lab.reshape(-1, *lab.shape[-2:]).long().cpu()
    H, W = l.shape[-2:]
    valid = (l >= 0) & (l < K) & (l != ignore)
    lp, vp = F.pad(l, (16,) * 4, value=-1), F.pad(valid, (16,) * 4, value=False)
    d2 = torch.full_like(l, 257)
    for dy in range(-16, 17):
        for dx in range(-16, 17):
            if dy * dy + dx * dx <= 256:
                q = (slice(None), slice(16 + dy, 16 + dy + H), slice(16 + dx, 16 + dx + W))
                d2 = torch.where(vp[q] & (lp[q] != l) & (dy * dy + dx * dx < d2), dy * dy + dx * dx, d2)
    return torch.where(valid, d2, 0).reshape(lab.shape).int(), valid.reshape(lab.shape)


def brute_erode(lab, K, ignore, r, fill):
    d2, valid = brute_d2(lab, K, ignore)
    return torch.where(valid & (d2 <= r * r), torch.full_like(lab.cpu(), fill), lab.cpu())


def blobs(B, H, W, K, seed, up=5):      # a coarse random class grid, upsampled x up
    c =torch.randint(0, K, (B, -(-H // up), -(-W // up)), generator=torch.Generator().manual_seed(seed))
    return c.repeat_interleave(up, 1).repeat_interleave(up, 2)[:, :H, :W].contiguous()


# "one_pixel": one class-1 pixel at (40, 40) of a class-0 image; the probes lie in other tiles
PROBES = {(40, 24): 256, (24, 39): 257, (28, 30): 244, (28, 29): 257}    # offsets (0,16) (16,1) (12,10) (12,11)


def _strips(dtype):        # class 0 | ignore, out-of-range labels | class 2: the strip is no boundary
    bad = [-100, -1, 3, 255] if dtype == torch.int64 else [1, 3, 255, 200]
    l = torch.zeros(1, 40, 50, dtype=torch.int64)
    l[..., 24:] = 2
    for i, v in enumerate(bad):
        l[..., 20 + i] = v
    return l, 3, bad[0]


# name -> (labels int64 [B, H, W], K, ignore_index); "per_image": two one-class images in front of a
# mixed one (no image sees the next)
CASES = {"small": lambda d: (blobs(1, 5, 7, 3, 0, up=2), 3, -100),
         "ragged": lambda d: (blobs(2, 33, 47, 6, 1), 6, -100),
         "interior": lambda d: (blobs(1, 64, 96, 5, 2), 5, -100),
         "per_image": lambda d: (blobs(3, 40, 40, 4, 3) * torch.tensor([0, 0, 1]).reshape(3, 1, 1)
                                 + torch.tensor([0, 1, 0]).reshape(3, 1, 1), 4, -100),
         "one_pixel": lambda d: (F.pad(torch.ones(1, 1, 1, dtype=torch.int64), (40, 29, 40, 29)), 2, -100),
         "strips": _strips,
         "k1": lambda d: (torch.zeros(1, 20, 20, dtype=torch.int64), 1, -100),
         "k16": lambda d: (blobs(2, 40, 70, 16, 4, up=3), 16, -100)}
_REF = {}


def reference(name, dtype):
    if (name, dtype) not in _REF:
        lab, K, ignore = CASES[name](dtype)
        lab = lab.to(dtype)
        lab = lab[0] if dtype == torch.uint8 and name == "small" else lab      # uint8 [H, W] too
        _REF[name, dtype] = (lab, K, ignore, *brute_d2(lab, K, ignore))
    return _REF[name, dtype]


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8], ids=["int64", "uint8"])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("dev", ["cpu", GPU])
def test_ops_match_brute_force(dev, name, dtype):
    ops = _ext.ops()
    lab, K, ignore, d2, valid = reference(name, dtype)
    fill = 255 if dtype == torch.uint8 else -100
    got = ops.label_dist2(lab.to(dev), K, ignore)
    assert got.dtype == torch.int32 and got.shape == lab.shape and torch.equal(got.cpu(), d2)
    for r in (0, 1, 3, 16):
        want = torch.where(valid & (d2 <= r * r), torch.full_like(lab, fill), lab)
        out = ops.label_erode(lab.to(dev), K, ignore, r, fill)
        assert out.dtype == lab.dtype and torch.equal(out.cpu(), want if r else lab), r
    if name == "one_pixel":
        assert {p: int(d2[0][p]) for p in PROBES} == PROBES
    if name in ("k1", "per_image"):
        assert int((d2[:2] if name == "per_image" else d2).min()) == 257       # far: nothing leaks in
    if name == "strips":
        assert int(d2[..., 20:24].max()) == 0 and int(d2[0, 5, 19]) == 25 and int(d2[0, 5, 24]) == 25
        assert torch.equal(out.cpu()[..., 20:24], lab[..., 20:24])             # (r = 16)


@pytest.mark.parametrize("dev", ["cpu", GPU])
def test_ops_refuse_bad_arguments(dev):
    ops, l = _ext.ops(), torch.zeros(1, 8, 8, dtype=torch.int64, device=dev)
    for bad in (lambda: ops.label_dist2(l, 17, -100), lambda: ops.label_dist2(l.int(), 3, -100),
                lambda: ops.label_erode(l, 3, -100, 17, -100), lambda: ops.label_erode(l, 3, -100, 3, 1),
                lambda: ops.label_erode(l.byte(), 3, -100, 3, 2), lambda: ops.label_dist2(l[:, :, ::2], 3, -100)):
        with pytest.raises(RuntimeError):
            bad()


# ------------------------------------------------------------------ the public interface
def _cfg(**kw):
    base = dict(model=ModelConfig(out_classes=6, depth=2), tile=32, batch_per_gpu=2, num_samples=6,
                test_holdout=4, impl="hip", log_every=0, log_dir=None)
    base.update(kw)
    return TrainConfig(**base).validate()


def _batch(dev, seed):
    return device_random_batch(2, 32, 6, dev, seed=seed)[0], blobs(2, 32, 32, 6, seed, up=8).to(dev)


class _Eroded:             # the held-out split with brute-force eroded labels
    def __init__(self, base, r):
        self.base, self.r = base, r

    def __len__(self):
        return len(self.base)

    def get(self, idx):
        x, y = self.base.get(idx)
        return x, brute_erode(y, 6, -100, self.r, -100).to(y.device)


@pytest.mark.parametrize("kw", [dict(), dict(fused_eval=False), dict(impl="torch", dtype="fp32")], ids=str)
def test_validate_eroded(kw):
    tr = Trainer(_cfg(eval_erode=3, **kw), device="cpu")
    got = tr.validate()
    x, y = tr._to_device(*_Eroded(tr.test_set, 3).get(list(range(4))))
    sums, cm = tr.model.eval().evaluate(x, y)
    want = metrics_of(cm)
    assert 0 < int(cm.sum()) < y.numel() and got["eval_erode"] == 3
    assert (got["val_pixel_acc"], got["val_iou"], got["val_miou"]) == (want["pixel_acc"], want["iou"], want["miou"])
    if tr.impl == "torch":  # one set of logits, 4096 positive terms summed in fp32 and in fp64: n 2^-24
        assert abs(got["val_loss"] - float(sums[0] / sums[2])) <= 4096 * 2.0 ** -24 * got["val_loss"]
    if tr.cfg.fused_eval and tr.impl == "hip":          # the same path on pre-eroded labels: the same bits
        tr.cfg.eval_erode = 0
        assert {**tr.validate(_Eroded(tr.test_set, 3)), "eval_erode": 3} == got
    tr.close()


def test_predict_eroded():
    sp = ScenePredictor(pc.make_model("d2_bilinear", "cpu"), 32, 16)
    scene, lab = pc.rand_scene(70, 52, 1, "cpu"), blobs(1, 70, 52, 3, 5, up=10)[0].byte()
    cm = sp.predict(scene, lab, erode=3)[1]
    assert torch.equal(cm, sp.predict(scene, brute_erode(lab, 3, -100, 3, 255))[1])
    assert 0 < int(cm.sum()) < int(sp.predict(scene, lab)[1].sum()) == 70 * 52
    with pytest.raises(ValueError):
        sp.predict(scene, lab, erode=17)


@pytest.mark.parametrize("kw", [dict(), dict(accum_steps=2, bn_window=2)], ids=str)
def test_train_erode_step(kw):
    """the step's loss is the loss on brute-force eroded labels, bit for bit"""
    losses = []
    for r in (2, 0):
        tr = Trainer(_cfg(train_erode=r, **kw), device="cpu")
        mbs = [_batch("cpu", s) for s in range(tr.cfg.accum_steps)]
        tr.train_step([(x, y if r else brute_erode(y, 6, -100, 2, -100)) for x, y in mbs])
        losses.append(tr.meter.reduce()["loss"])
        tr.close()
    assert losses[0] == losses[1] and losses[0] > 0


def test_config_and_radius_zero(monkeypatch):
    cfg = config_from_args(add_config_args(argparse.ArgumentParser()).parse_args(["--eval-erode", "3", "--train-erode", "2"]))
    assert (cfg.eval_erode, cfg.train_erode) == (3, 2)
    for bad in (dict(eval_erode=17), dict(train_erode=17), dict(train_erode=-1),
                dict(eval_erode=3, model=ModelConfig(dims=3)), dict(train_erode=1, model=ModelConfig(dims=3))):
        with pytest.raises(ValueError):
            _cfg(**bad)
    monkeypatch.setattr(boundary, "erode_labels", None)    # both radii 0 (the default): a call would raise
    tr = Trainer(_cfg(), device="cpu")
    assert (tr.cfg.eval_erode, tr.cfg.train_erode) == (0, 0) and tr.validate()["eval_erode"] == 0
    tr.train_step([_batch("cpu", 0)])
    tr.close()
    ScenePredictor(pc.make_model("d2_bilinear", "cpu"), 32, 16).predict(
        pc.rand_scene(40, 40, 1, "cpu"), torch.zeros(40, 40, dtype=torch.uint8))


@pytest.mark.gpu
def test_hip_graph_with_train_erode_matches_eager():
    """3 eager steps (warm-up + capture) and 2 replays against 5 eager steps: bit for bit"""
    out = []
    for graph in (False, True):
        tr = Trainer(_cfg(train_erode=2, hip_graph=graph, num_samples=1, test_holdout=0), device="cuda")
        batches = [_batch(tr.device, s) for s in range(3)]
        for i in range(5):
            tr.train_step([batches[i % 3]])
        assert not graph or "last" in tr._graphs, "step was not captured"
        out.append((tr.flat.param_buf.clone(), torch.as_tensor(tr.meter.reduce()["loss"])))
        tr.close()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and float(out[0][1]) > 0
