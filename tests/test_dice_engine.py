"""The soft-Dice term through the engine (against the fp32 stock modules computing the same
formula, the criterion of ``test_engine_cpu.py``), the captured step, and the configuration."""
import argparse
import json
import statistics

import pytest
import torch
import torch.nn.functional as F

LAM = 0.5
GPU = pytest.param("cuda", marks=pytest.mark.gpu)


def _grads(dev, hip, autocast=False):
    from ddlpc.models import UNet
    g = torch.Generator().manual_seed(7)
    x = torch.rand((2, 3, 32, 32), generator=g).to(dev)
    y = torch.randint(0, 6, (2, 32, 32), generator=g)
    y[torch.rand((2, 32, 32), generator=g) < 0.1] = -100
    torch.manual_seed(0)
    m = UNet(out_classes=6, depth=2, width_divisor=2).train().to(dev)
    m = m.to_hip() if hip else m
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        loss, correct = m.loss_and_correct(x, y.to(dev), dice_weight=LAM, dice_smooth=1.0)
    loss.backward()
    grads = [(n, p.grad.detach().flatten().cpu()) for n, p in m.named_parameters()]
    return float(loss.detach()), int(correct), m.dice_terms(), grads


@pytest.mark.parametrize("dev", ["cpu", GPU])
def test_engine_dice_matches_fp32_autograd(dev):
    l0, c0, t0, g0 = _grads("cpu", False)
    _, _, _, ga = _grads("cpu", False, autocast=True)
    l1, c1, t1, ge = _grads(dev, True)
    assert abs(l1 - l0) < 2e-3 * abs(l0) and abs(c1 - c0) <= 0.01 * 2 * 32 * 32
    assert all(abs(a - b) < 2e-3 * abs(b) for a, b in zip(t1, t0)) and abs(t1[1] + LAM * t1[0] - l1) < 1e-5
    cos_e, cos_a = [], []
    for (name, a), (_, b), (_, e) in zip(g0, ga, ge):
        if name.endswith(".bias") and ("double_conv.0" in name or "double_conv.3" in name):
            assert torch.count_nonzero(e) == 0, name                  # conv bias feeding a training BN
            continue
        ce_, ca = float(F.cosine_similarity(a, e, dim=0)), float(F.cosine_similarity(a, b, dim=0))
        assert ce_ >= ca - 0.15, (name, ce_, ca)
        cos_e.append(ce_)
        cos_a.append(ca)
    assert statistics.median(cos_e) >= statistics.median(cos_a) - 0.04


def _cfg(**kw):
    from ddlpc.config import ModelConfig, TrainConfig
    base = dict(model=ModelConfig(out_classes=6, depth=2), tile=32, batch_per_gpu=2, num_samples=1,
                test_holdout=0, impl="hip", log_every=0, log_dir=None, dice_weight=LAM)
    base.update(kw)
    return TrainConfig(**base)


@pytest.mark.gpu
def test_hip_graph_with_dice_matches_eager():
    """3 eager steps (warm-up + capture) and 3 replays against 6 eager steps: bit for bit"""
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    out = []
    for graph in (False, True):
        tr = Trainer(_cfg(hip_graph=graph).validate(), device="cuda")
        batches = [device_random_batch(2, 32, 6, tr.device, seed=s) for s in range(3)]
        for i in range(6):
            tr.train_step([batches[i % 3]])
        assert not graph or "last" in tr._graphs, "step was not captured"
        out.append((tr.flat.param_buf.clone(), tr.meter.reduce()["loss"], tr.model._engine.dice_table.clone()))
        tr.close()
    for a, b in zip(*out):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))


def test_config_cli_checkpoint(tmp_path):
    from ddlpc.config import add_config_args, config_from_args
    from ddlpc.train.checkpoint import load_checkpoint
    from ddlpc.train.trainer import Trainer
    cfg = config_from_args(add_config_args(argparse.ArgumentParser()).parse_args(
        ["--dice-weight", "0.5", "--dice-smooth", "2"]))
    assert cfg.dice_weight == 0.5 and cfg.dice_smooth == 2.0
    for bad in (dict(dice_weight=-1.0), dict(dice_smooth=0.0), dict(bn_window=4, accum_steps=4)):
        with pytest.raises(ValueError):
            _cfg(**bad).validate()
    tr = Trainer(_cfg(dice_smooth=2.0, accum_steps=2, bn_window=-1, ckpt_dir=str(tmp_path), num_samples=8,
                      log_every=1, log_dir=str(tmp_path)).validate(), device="cpu")
    assert tr._window_size(2) == 0                                    # auto: per-micro-batch passes
    tr.fit()
    blob = load_checkpoint(tr.save())
    assert blob["config"]["dice_weight"] == LAM and blob["config"]["dice_smooth"] == 2.0
    tr.close()
    recs = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    steps = [r for r in recs if "images_per_s" in r]
    assert steps and all(0 < r["dice"] < 1 and r["ce"] > 0 for r in steps)


def test_dice_off_trace_equals_golden(monkeypatch):
    import schedule_cases as sc
    from ddlpc.models import UNet
    plain = UNet.loss_and_correct
    monkeypatch.setattr(UNet, "loss_and_correct",
                        lambda self, x, y, **kw: plain(self, x, y, dice_weight=0.0, dice_smooth=1.0, **kw))
    with sc.eight_cus():
        r = sc._run(sc.BY_NAME["default"], False, "cpu")
    assert r.sha256 == sc.golden()[sc.key_id("default", False)]["sha256"]
