"""Learning-rate schedule, gradient-norm clipping and decoupled weight decay from the public
interface down: ``TrainConfig`` fields and their flags, ``validate()``, checkpoints from before
the fields existed, and the trainer on the CPU kernels (logged ``lr`` / ``grad_norm`` /
``clip_coef``, resume in the middle of a schedule, two gloo ranks under clipping); a ``gpu``-marked
test replays the scheduled step in a hipGraph.
"""
import argparse
import json
import math

import pytest
import torch

from dist_utils import run

SCHED = dict(lr_schedule="poly", lr_warmup_steps=2, max_grad_norm=0.25, decoupled_weight_decay=True,
             weight_decay=0.01)


def _cfg(**kw):
    from ddlpc.config import ModelConfig, TrainConfig
    base = dict(model=ModelConfig(out_classes=6, depth=2), tile=32, num_samples=8, test_holdout=0,
                batch_per_gpu=2, accum_steps=1, epochs=2, log_every=1, log_dir=None, impl="hip",
                shuffle=False, timeout_s=60)
    base.update(kw)
    return TrainConfig(**base)


# ------------------------------------------------------------------ config and flags
def test_flags_round_trip():
    from ddlpc.config import add_config_args, config_from_args
    p = add_config_args(argparse.ArgumentParser())
    cfg = config_from_args(p.parse_args(
        ["--lr-schedule", "cosine", "--lr-warmup-steps", "7", "--lr-total-steps", "90", "--lr-min", "1e-5",
         "--lr-poly-power", "1.5", "--max-grad-norm", "2.5", "--decoupled-weight-decay", "true",
         "--weight-decay", "0.01"]))
    assert (cfg.lr_schedule, cfg.lr_warmup_steps, cfg.lr_total_steps, cfg.lr_min, cfg.lr_poly_power,
            cfg.max_grad_norm, cfg.decoupled_weight_decay) == ("cosine", 7, 90, 1e-5, 1.5, 2.5, True)
    assert cfg.scheduled
    again = type(cfg).from_dict(json.loads(json.dumps(cfg.to_dict())))
    assert again.to_dict() == cfg.to_dict()
    plain = config_from_args(p.parse_args([]))
    assert not plain.scheduled and plain.lr_schedule == "constant" and plain.max_grad_norm == 0.0


@pytest.mark.parametrize("bad", [dict(lr_schedule="linear"), dict(lr_warmup_steps=-1), dict(lr_total_steps=-1),
                                 dict(lr_min=-1e-6), dict(max_grad_norm=-1.0), dict(lr_min=2e-3),
                                 dict(lr_poly_power=0.0), dict(lr_poly_power=-1.0)],
                         ids=lambda d: "{}={}".format(*next(iter(d.items()))))
def test_validate_refuses(bad):
    with pytest.raises(ValueError):
        _cfg(**bad).validate()


def test_config_without_the_keys_loads():
    """a checkpoint's config from before these fields: the defaults apply (plain Adam)"""
    from ddlpc.config import TrainConfig
    d = _cfg().to_dict()
    for k in ("lr_schedule", "lr_warmup_steps", "lr_total_steps", "lr_min", "lr_poly_power", "max_grad_norm",
              "decoupled_weight_decay"):
        del d[k]
    cfg = TrainConfig.from_dict(d)
    assert not cfg.scheduled and cfg.lr_schedule == "constant" and cfg.decoupled_weight_decay is False


def test_defaults_keep_todays_optimizer():
    """every new argument at its default: no table, no partials — today's code path"""
    from ddlpc.train.trainer import Trainer
    tr = Trainer(_cfg(), device="cpu")
    assert not tr.optimizer.scheduled and tr.optimizer._partial is None
    with pytest.raises(RuntimeError):
        tr.optimizer.last_stats()
    tr.close()


# ------------------------------------------------------------------ trainer on the CPU kernels
def test_trainer_logs_schedule_and_clipping(tmp_path):
    from ddlpc.train.trainer import Trainer
    tr = Trainer(_cfg(log_dir=str(tmp_path / "log"), **SCHED), device="cpu")
    opt = tr.optimizer
    assert opt.scheduled and opt.total_steps == 8 and opt.decoupled      # auto: 2 epochs x 4 steps
    tr.fit()
    tr.close()
    recs = [r for r in map(json.loads, open(tmp_path / "log" / "metrics.jsonl")) if "step" in r and "lr" in r]
    assert [r["step"] for r in recs] == list(range(1, 9))
    for r in recs:
        want = float(torch.tensor(opt.lr_at(r["step"]), dtype=torch.float32))
        assert r["lr"] == want, (r["step"], r["lr"], want)
        assert r["grad_norm"] > 0 and 0 < r["clip_coef"] <= 1
    assert recs[0]["clip_coef"] < 1 and recs[0]["grad_norm"] > SCHED["max_grad_norm"]
    assert recs[0]["lr"] < recs[1]["lr"] and recs[-1]["lr"] < recs[2]["lr"]


def test_resume_continues_the_schedule(tmp_path):
    """saved at step 3 and resumed: the parameters at step 6 are those of the uninterrupted run"""
    from ddlpc.train.trainer import Trainer
    kw = dict(lr_total_steps=8, **SCHED)
    full = Trainer(_cfg(max_steps=6, **kw), device="cpu")
    full.fit()
    want = full.flat.param_buf.clone()
    full.close()
    a = Trainer(_cfg(max_steps=3, ckpt_dir=str(tmp_path / "ck"), **kw), device="cpu")
    a.fit()
    a.close()
    b = Trainer(_cfg(max_steps=6, ckpt_dir=str(tmp_path / "ck"), resume="auto", **kw), device="cpu")
    assert b.step_count == 3 and float(b.optimizer._dev_scal[0]) == 3.0
    b.fit()
    assert b.step_count == 6 and float(b.optimizer._dev_scal[0]) == 6.0
    assert b.optimizer.last_stats()["lr"] == float(torch.tensor(b.optimizer.lr_at(6), dtype=torch.float32))
    assert torch.equal(b.flat.param_buf, want)
    b.close()


def _clipped_ranks(rank, world):
    from ddlpc.parallel import params_checksum
    from ddlpc.train.trainer import Trainer
    tr = Trainer(_cfg(check_consistency_every=1, bucket_mb=0.05, **SCHED), device="cpu")
    tr.fit()
    out = {"checksum": float(params_checksum(tr.model)), "steps": tr.step_count, **tr.optimizer.last_stats()}
    tr.close()
    return out


def test_two_gloo_ranks_stay_identical_under_clipping():
    res = run(_clipped_ranks, 2, ())
    assert res[0]["steps"] == res[1]["steps"] > 0
    assert res[0] == res[1] and res[0]["grad_norm"] > 0


# ------------------------------------------------------------------ hipGraph
@pytest.mark.gpu
def test_hip_graph_replays_the_schedule():
    """cosine with warm-up 2 of 8 and clipping, eight steps with hip_graph off and on: parameters,
    both moments and the device table are bit-identical after every step, and the table's lr
    follows lr_at(t) through the replayed steps (nothing step-dependent is baked into the graph)"""
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    out = []
    for graph in (False, True):
        tr = Trainer(_cfg(tile=64, batch_per_gpu=4, num_samples=1, log_every=0, hip_graph=graph,
                          lr_schedule="cosine", lr_warmup_steps=2, lr_total_steps=8, lr_min=1e-5,
                          max_grad_norm=0.5, weight_decay=0.01, decoupled_weight_decay=True), device="cuda")
        batches = [device_random_batch(4, 64, 6, tr.device, seed=s) for s in range(3)]
        opt, steps = tr.optimizer, []
        for i in range(8):                       # 3 eager warm-up steps + capture, then replays
            tr.train_step([batches[i % 3]])
            sc = opt._dev_scal.cpu().clone()
            assert float(sc[0]) == i + 1 == opt.step_count
            lr_t = opt.lr_at(i + 1)               # (one fp32 ulp: the device's cos is not correctly rounded)
            assert abs(float(sc[3]) - lr_t) <= 2.0 ** (math.frexp(lr_t)[1] - 24), (i + 1, float(sc[3]), lr_t)
            steps.append((tr.flat.param_buf.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), sc))
        if graph:
            assert "last" in tr._graphs, "step was not captured"
        out.append(steps)
        tr.close()
    assert any(float(s[3][5]) < 1.0 for s in out[0]), "bad case: no step was clipped"
    for i, (a, b) in enumerate(zip(*out)):
        for name, x, y in zip(("p", "m", "v", "scal"), a, b):
            assert torch.equal(x, y), (f"{name} differs at step {i + 1}", float((x - y).abs().max()))
