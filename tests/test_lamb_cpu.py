"""``test_lamb_gpu.py`` run against the CPU kernels (the same text with ``DEV = "cpu"``), and
``optimizer="lamb"`` from the public interface down on the CPU engine."""
import json
import os

import pytest
import torch

import lamb_cases as lc
from test_sched_trainer import _cfg

_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_lamb_gpu.py")
_src = open(_path).read()
assert 'DEV = "cuda"' in _src and "pytestmark = pytest.mark.gpu" in _src
_src = _src.replace("pytestmark = pytest.mark.gpu", "pytestmark = []", 1).replace('DEV = "cuda"', 'DEV = "cpu"', 1)
exec(compile(_src, _path, "exec"), globals())
del globals()["test_same_bits_twice_and_captured"]        # (a hipGraph: GPU only)
LAMB = dict(optimizer="lamb", lr_schedule="poly", lr_warmup_steps=2, lr_total_steps=8, max_grad_norm=0.25, weight_decay=0.01)


def test_trainer_logs_trust_ratios(tmp_path):
    from ddlpc.train.trainer import Trainer
    with pytest.raises(ValueError):
        _cfg(decoupled_weight_decay=True, **LAMB).validate()
    tr = Trainer(_cfg(log_dir=str(tmp_path / "log"), **LAMB), device="cpu")
    assert type(tr.optimizer).__name__ == "FlatLamb" and not all(tr.optimizer.adapted)
    tr.fit()
    tr.close()
    recs = [r for r in map(json.loads, open(tmp_path / "log" / "metrics.jsonl")) if "trust_min" in r]
    assert [r["step"] for r in recs] == list(range(1, 9))
    for r in recs:
        assert 0 < r["trust_min"] < r["trust_max"] and r["grad_norm"] > 0 and 0 < r["clip_coef"] <= 1
        assert r["lr"] == lc.f32(tr.optimizer.lr_at(r["step"]))


def test_resume_and_adam_format(tmp_path):
    """saved at step 3 and resumed: bit-identical parameters at step 6; the checkpoint loads into torch.optim.Adam"""
    from ddlpc.train.trainer import Trainer
    want = None
    for kw in (dict(max_steps=6), dict(max_steps=3, ckpt_dir=str(tmp_path)),
               dict(max_steps=6, ckpt_dir=str(tmp_path), resume="auto")):
        tr = Trainer(_cfg(**LAMB, **kw), device="cpu")
        assert tr.step_count == (3 if "resume" in kw else 0) == float(tr.optimizer._dev_scal[0])
        tr.fit()
        want = tr.flat.param_buf.clone() if want is None else want
        tr.close()
    assert torch.equal(tr.flat.param_buf, want)
    adam = torch.optim.Adam(tr.model.parameters())
    adam.load_state_dict(torch.load(tmp_path / "ckpt_3.pt", weights_only=True)["optimizer"])
    st = adam.state_dict()["state"][0]
    assert float(st["step"]) == 3 and float(st["exp_avg"].abs().sum()) > 0
