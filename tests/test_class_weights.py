"""Class-weighted cross-entropy (``CrossEntropyLoss(weight=...)``) from the public interface
down: the engine's ``loss_and_correct(..., class_weight=)`` against the stock modules with
``F.cross_entropy(weight=)`` (CPU kernels here, a ``gpu``-marked twin on the gfx950 kernels),
``TrainConfig.class_weights`` / ``--class-weights`` (a list, ``median_freq``, bad inputs), and
the trainer (resolved weights in ``metrics.jsonl`` and the checkpoint; the torch fp32 path).

The engine comparison holds loss, hit count, running statistics and gradients to the
tolerances of ``test_engine_cpu.py::test_engine_on_cpu_matches_fp32_autograd`` (taken from
there): loss 2e-3 relative, hits 1 % of the pixels, buffers 5e-3, each gradient's cosine to fp32
autograd at most 0.15 below the bf16-autocast run's and the median at most 0.04 below it.
"""
import json
import statistics

import numpy as np
import pytest
import torch
import torch.nn.functional as F

WEIGHTS = [0.3, 0.0, 3.0, 0.7, 1.9, 1.0]


def _model(seed=0):
    """the smallest supported U-Net: depth 2 (a 32-channel head), 6 classes"""
    from ddlpc.models import UNet
    torch.manual_seed(seed)
    return UNet(out_classes=6, depth=2).train()


def _batch():
    g = torch.Generator().manual_seed(7)
    x = torch.rand((4, 3, 32, 32), generator=g)
    y = torch.randint(0, 6, (4, 32, 32), generator=g)
    y[0, :3] = -100                                   # some ignored pixels
    return x, y


def _stock(model, x, y, w, groups, autocast=False):
    """stock modules; bn_groups = G: G micro-batches with their own BatchNorm statistics, one
    loss over all their pixels"""
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        parts = x.chunk(groups) if groups > 1 else [x]
        logits = torch.cat([model.forward_torch(p) for p in parts])
        loss = F.cross_entropy(logits.float(), y, weight=w, ignore_index=-100)
    correct = int((logits.detach().argmax(1) == y).sum())
    loss.backward()
    return float(loss.detach()), correct, [p.grad.detach().flatten().clone() for p in model.parameters()]


def _engine_vs_autograd(dev, head_apply, head_fused_fwd, groups):
    x, y = _batch()
    w = torch.tensor(WEIGHTS)
    ref = _model()
    l0, c0, g0 = _stock(ref, x, y, w, groups)
    _, _, ga = _stock(_model(), x, y, w, groups, autocast=True)
    eng = _model().to(dev).to_hip()
    e = eng._engine
    e.head_apply, e.head_fused_fwd, e.bn_groups = head_apply, head_fused_fwd, groups
    loss, correct = eng.loss_and_correct(x.to(dev), y.to(dev), -100, w.to(dev))
    loss.backward()
    l1, c1 = float(loss.detach()), int(correct)
    ge = [p.grad.detach().flatten().cpu().clone() for p in eng.parameters()]
    assert abs(l1 - l0) < 2e-3 * abs(l0), (l1, l0)
    assert abs(c1 - c0) <= 0.01 * y.numel()
    for b0, b1 in zip(ref.buffers(), eng.buffers()):
        if b0.dtype.is_floating_point:
            assert torch.allclose(b0, b1.cpu(), atol=5e-3, rtol=5e-3)
        else:
            assert torch.equal(b0, b1.cpu())
    cos_e, cos_a = [], []
    for (name, _), a, b, g in zip(ref.named_parameters(), g0, ga, ge):
        if name.endswith(".bias") and ("double_conv.0" in name or "double_conv.3" in name):
            assert torch.count_nonzero(g) == 0, name      # conv bias feeding a training BN
            continue
        ce, ca = float(F.cosine_similarity(a, g, dim=0)), float(F.cosine_similarity(a, b, dim=0))
        assert ce >= ca - 0.15, (name, ce, ca)
        cos_e.append(ce)
        cos_a.append(ca)
    assert statistics.median(cos_e) >= statistics.median(cos_a) - 0.04


SCHEDULES = [(True, True, 0), (True, False, 0), (False, True, 0), (False, False, 0), (True, True, 2)]
_SID = [f"apply{int(a)}-fused{int(f)}-groups{g}" for a, f, g in SCHEDULES]


@pytest.mark.parametrize("head_apply,head_fused_fwd,groups", SCHEDULES, ids=_SID)
def test_engine_matches_weighted_autograd_cpu(head_apply, head_fused_fwd, groups):
    _engine_vs_autograd("cpu", head_apply, head_fused_fwd, groups)


@pytest.mark.gpu
@pytest.mark.parametrize("head_apply,head_fused_fwd,groups", SCHEDULES, ids=_SID)
def test_engine_matches_weighted_autograd_gpu(head_apply, head_fused_fwd, groups):
    _engine_vs_autograd("cuda", head_apply, head_fused_fwd, groups)


def test_engine_rejects_bad_weight_tensor():
    x, y = _batch()
    eng = _model().to_hip()
    for bad in (torch.ones(5), torch.ones(6, dtype=torch.float64), torch.ones(1, 6)):
        with pytest.raises(ValueError):
            eng.loss_and_correct(x, y, -100, bad)


def test_stock_path_takes_weights():
    x, y = _batch()
    m = _model()
    w = torch.tensor(WEIGHTS)
    loss, _ = m.loss_and_correct(x, y, class_weight=w)
    want = F.cross_entropy(m.forward_torch(x).float(), y, weight=w)
    assert torch.equal(loss.detach(), want.detach())


# ------------------------------------------------------------------ config / CLI
def _cfg(**kw):
    from ddlpc.config import ModelConfig, TrainConfig
    base = dict(model=ModelConfig(out_classes=6, depth=2), tile=32, num_samples=8, test_holdout=2,
                batch_per_gpu=2, accum_steps=1, epochs=1, log_every=0, log_dir=None, impl="hip",
                timeout_s=60)
    base.update(kw)
    return TrainConfig(**base)


def test_config_accepts_list_and_median_freq(tmp_path):
    from ddlpc.config import TrainConfig, parse_class_weights
    c = _cfg(class_weights="1,2,0.5,0,3,1").validate()
    assert parse_class_weights(c.class_weights, 6) == [1.0, 2.0, 0.5, 0.0, 3.0, 1.0]
    # a YAML / JSON list, through the (de)serialisation round trip
    d = c.to_dict()
    d["class_weights"] = [1, 2, 0.5, 0, 3, 1]
    c2 = TrainConfig.from_dict(d)
    assert parse_class_weights(c2.class_weights, 6) == [1.0, 2.0, 0.5, 0.0, 3.0, 1.0]
    assert isinstance(c2.to_dict()["class_weights"], str)
    assert _cfg(class_weights=None).validate().class_weights is None
    c3 = _cfg(class_weights="median_freq", data="scene_dir", data_dir=str(tmp_path)).validate()
    assert c3.class_weights == "median_freq"


@pytest.mark.parametrize("spec,kw", [
    ("1,2,3", {}),                                    # wrong length
    ("1,2,3,4,5,6,7", {}),
    ("1,-1,1,1,1,1", {}),                             # negative
    ("0,0,0,0,0,0", {}),                              # all zero
    ("1,nan,1,1,1,1", {}),
    ("1,inf,1,1,1,1", {}),
    ("balanced", {}),                                 # neither a list nor a known mode
    ("median_freq", {"data": "synthetic"}),           # needs label files
])
def test_config_rejects_bad_class_weights(spec, kw):
    with pytest.raises(ValueError):
        _cfg(class_weights=spec, **kw).validate()


def test_cli_flag(capsys):
    from ddlpc.cli import main
    assert main(["config", "--class-weights", "1,2,0.5,0,3,1"]) == 0
    assert json.loads(capsys.readouterr().out)["class_weights"] == "1,2,0.5,0,3,1"
    with pytest.raises(ValueError):
        main(["config", "--class-weights", "1,2"])
    with pytest.raises(ValueError):
        main(["config", "--class-weights", "median_freq"])          # data defaults to synthetic


# ------------------------------------------------------------------ trainer
def _write_scenes(path, n=5, size=40, seed=3, vary=True, outside=False):
    """n scenes (vary: of unequal sizes) with unequal class shares and one class absent;
    outside: 2 % of the labels are 255, outside [0, 6)"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    labs = []
    for i in range(n):
        h, w = (size + 3 * i, size + 5) if vary else (size, size)
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(path / f"s_{i:03d}.png")
        y = rng.choice([0, 1, 2, 4, 5, 255 if outside else 0], size=(h, w),
                       p=[0.5, 0.25, 0.12, 0.08, 0.03, 0.02]).astype(np.uint8)
        np.save(path / f"s_{i:03d}_label.npy", y)
        labs.append(y)
    return labs


def _median_freq(labs, K):
    n = np.zeros(K, dtype=np.float64)
    for y in labs:
        for k in range(K):
            n[k] += np.count_nonzero(y == k)
    f = n / n.sum()
    med = np.median(f[n > 0])
    return np.where(n > 0, med / np.where(n > 0, f, 1.0), 1.0).astype(np.float32)


@pytest.mark.parametrize("data,outside", [("scene_dir", False), ("scene_dir", True),
                                          ("vaihingen_dir", False)])
def test_median_freq_from_training_split(tmp_path, data, outside):
    """median_freq equals the formula on the TRAINING scenes' labels (the held-out ones and the
    labels outside [0, K) not counted; the absent class gets 1.0), lands in metrics.jsonl and in
    the checkpoint, and the trainer trains with it (not on the label files with values outside
    [0, K): no loss accepts those)"""
    from ddlpc.train.checkpoint import load_checkpoint
    from ddlpc.train.trainer import Trainer
    d = tmp_path / "scenes"
    d.mkdir()
    # (vaihingen_dir: pre-cut tiles of one size)
    labs = _write_scenes(d, outside=outside) if data == "scene_dir" else _write_scenes(d, size=32, vary=False)
    want = _median_freq(labs[:-2], 6)
    assert want[3] == 1.0 and len(set(want.tolist())) > 3
    log, ck = tmp_path / "log", tmp_path / "ck"
    tr = Trainer(_cfg(data=data, data_dir=str(d), class_weights="median_freq", test_holdout=2,
                      log_dir=str(log), ckpt_dir=str(ck)), device="cpu")
    assert tr.class_weight.dtype == torch.float32
    assert np.array_equal(tr.class_weight.numpy(), want), (tr.class_weight, want)
    assert np.array_equal(np.asarray(tr.class_weights, dtype=np.float32), want)
    if not outside:
        x, y = tr.train_set.get([0, 1])
        tr.train_step([(x, y)])
        m = tr.meter.reduce()
        assert m["loss"] == m["loss"]
    path = tr.save()
    tr.close()
    recs = [json.loads(l) for l in open(log / "metrics.jsonl")]
    logged = [r["class_weights"] for r in recs if "class_weights" in r]
    assert len(logged) == 1 and np.array_equal(np.asarray(logged[0], dtype=np.float32), want)
    blob = load_checkpoint(path)
    assert np.array_equal(np.asarray(blob["class_weights"], dtype=np.float32), want)
    assert blob["config"]["class_weights"] == "median_freq"


def test_trainer_list_weights_and_torch_fp32_path(tmp_path):
    """a configured list reaches the loss on the stock fp32 path: the first step's logged loss is
    F.cross_entropy(weight=) of the same batch on the same initial weights"""
    from ddlpc.train.trainer import Trainer
    spec = "0.3,0,3,0.7,1.9,1"
    tr = Trainer(_cfg(impl="torch", dtype="fp32", class_weights=spec, log_dir=str(tmp_path / "log")),
                 device="cpu")
    assert tr.impl == "torch" and tr.class_weights == [0.3, 0.0, 3.0, 0.7, 1.9, 1.0]
    x, y = tr.train_set.get([0, 1])
    with torch.no_grad():
        want = F.cross_entropy(tr.model.forward_torch(x).float(), y, weight=torch.tensor(tr.class_weights))
        plain = F.cross_entropy(tr.model.forward_torch(x).float(), y)
    tr.meter.reset()
    tr.train_step([(x, y)])
    got = tr.meter.reduce()["loss"]
    assert abs(got - float(want)) < 1e-5 * abs(float(want)) and abs(got - float(plain)) > 1e-3
    losses = [got]
    for _ in range(5):
        tr.meter.reset()
        tr.train_step([(x, y)])
        losses.append(tr.meter.reduce()["loss"])
    assert losses[-1] < losses[0]
    tr.close()


def test_trainer_without_weights_logs_nothing(tmp_path):
    from ddlpc.train.checkpoint import load_checkpoint
    from ddlpc.train.trainer import Trainer
    tr = Trainer(_cfg(log_dir=str(tmp_path / "log"), ckpt_dir=str(tmp_path / "ck")), device="cpu")
    assert tr.class_weight is None and tr.class_weights is None
    path = tr.save()
    tr.close()
    assert "class_weights" not in open(tmp_path / "log" / "metrics.jsonl").read()
    assert "class_weights" not in load_checkpoint(path)


def _three_steps(dev, spec):
    from ddlpc.train.trainer import Trainer
    torch.manual_seed(0)
    tr = Trainer(_cfg(class_weights=spec), device=dev)
    x, y = tr.train_set.get([0, 1])
    for _ in range(3):
        tr.train_step([(x, y)])
    p = torch.cat([q.detach().flatten().cpu() for q in tr.model.parameters()])
    b = torch.cat([q.detach().float().flatten().cpu() for q in tr.model.buffers()])
    tr.close()
    return p, b


def test_all_ones_training_is_bit_identical_cpu():
    """three optimizer steps with all-ones weights = three steps without weights, bit for bit"""
    p0, b0 = _three_steps("cpu", None)
    p1, b1 = _three_steps("cpu", "1,1,1,1,1,1")
    assert torch.equal(p0, p1) and torch.equal(b0, b1)


@pytest.mark.gpu
def test_all_ones_training_is_bit_identical_gpu():
    p0, b0 = _three_steps("cuda", None)
    p1, b1 = _three_steps("cuda", "1,1,1,1,1,1")
    assert torch.equal(p0, p1) and torch.equal(b0, b1)


@pytest.mark.gpu
def test_hip_graph_with_weights_matches_eager():
    """cfg.hip_graph with class weights (a persistent device tensor read by the captured
    kernels): the replayed steps reproduce the eager ones bit for bit, and differ from the
    unweighted run"""
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    out = []
    for graph, spec in ((False, "0.3,0,3,0.7,1.9,1"), (True, "0.3,0,3,0.7,1.9,1"), (False, None)):
        tr = Trainer(_cfg(tile=64, batch_per_gpu=4, num_samples=1, test_holdout=0, hip_graph=graph,
                          class_weights=spec), device="cuda")
        batches = [device_random_batch(4, 64, 6, tr.device, seed=s) for s in range(3)]
        losses = []
        for i in range(6):                       # 3 eager warm-up steps + capture, then replays
            tr.train_step([batches[i % 3]])
            losses.append(tr.meter.reduce()["loss"])
            tr.meter.reset()
        if graph:
            assert "last" in tr._graphs, "step was not captured"
        out.append((tr.flat.param_buf.clone(), losses))
        tr.close()
    (p0, l0), (p1, l1), (p2, l2) = out
    assert torch.equal(p0, p1), float((p0 - p1).abs().max())
    assert l0 == l1
    assert not torch.equal(p0, p2) and l0[0] != l2[0]
