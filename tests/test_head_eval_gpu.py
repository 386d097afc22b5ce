"""The evaluation head ``head_eval`` (``csrc/head_ce.hip``) against an fp64 reference formed from
the bf16-rounded activation, and ``UNet.evaluate`` / ``Trainer.validate`` against the logits path
(docs/TESTING.md, "Evaluation head").  ``num_cus()`` is pinned to 8.  P0 runs tail lanes and waves
with fewer steps than the look-ahead, at PLOOP every persistent loop takes a second trip, at PTINY
most workgroups are idle.
"""
import argparse

import pytest
import torch

import exact_cases as xc
import head_cases as hc

pytestmark = pytest.mark.gpu

DEV = "cuda"
P0, PLOOP, PTINY = 16 * 37 + 5, 16 * 800 + 5, 7
GRID = [(C, K, d) for C in (8, 16, 32, 64) for K in (2, 6, 16) for d in (0, 1)]
# Gaussian cases: hc.make's seed 7 except where its reference has a pixel whose top-2 gap lies within
# 2 eps (test_loss_gauss asserts on the reference alone that there is none)
SEEDS = {(16, 16, 0): 9}


@pytest.fixture(scope="module")
def ops():
    o = xc.ops()
    if DEV != "cuda":
        yield o
        return
    try:
        o.set_cu_reserve(int(o.set_cu_reserve(0)) - 8)
        assert int(o.set_cu_reserve(-1)) == 8
        yield o
    finally:
        o.set_cu_reserve(0)


def inputs(mode, C, K, defer, P):
    c = dict(mode=mode, N=1, H=1, W=P, C=C, K=K, defer=int(defer))
    c.update(dict(tie=(0, K - 1)) if mode == "tie" else dict(spread=0.3, seed=SEEDS.get((C, K, defer), 7)))
    cs = hc.make(c)
    g = torch.Generator().manual_seed(11)
    lab = cs.lab.reshape(-1).clone()
    lab[lab == 1] = 0                                                 # class 1 is absent
    lab[torch.rand(P, generator=g) < 0.1] = cs.ign
    lab[torch.rand(P, generator=g) < 0.02] = 255                      # out of range
    return cs, lab


def reference(cs, lab):       # fp64, from the bf16-rounded activation and the fp32 weights
    r = hc.Ref()
    A, W, b = hc._act(cs), cs.Wh.double(), cs.bh.double()
    z = A @ W.t() + b
    r.eps = 2.0 ** -15 * (1 + (A.abs() @ W.abs().t() + b.abs()).max(1).values)
    top = z.topk(2, dim=1).values
    r.on = (lab >= 0) & (lab < cs.K) & (lab != cs.ign)
    r.near = int((r.on & (top[:, 0] - top[:, 1] <= 2 * r.eps)).sum())
    y, am = lab[r.on], hc._first_max(z)[r.on]
    r.cm = torch.bincount(y * cs.K + am, minlength=cs.K ** 2).reshape(cs.K, cs.K)
    r.count, r.hits = int(r.on.sum()), int((am == y).sum())
    r.loss_px = torch.logsumexp(z[r.on], 1) - z[r.on].gather(1, y[:, None])[:, 0]
    # the per-pixel logit bound over the counted pixels + the fp32 row sums of at most P + 256 terms
    r.bound = float(r.eps[r.on].sum()) + (cs.P + 256) * 2.0 ** -24 * float(r.loss_px.abs().sum())
    return r


def run(o, cs, lab, out=None, sl=slice(None)):
    t = lambda v: None if v is None else v.to(DEV)
    sums, cm = out or (torch.zeros(3, dtype=torch.float64, device=DEV),
                       torch.zeros(cs.K, cs.K, dtype=torch.int64, device=DEV))
    o.head_eval(t(cs.y.reshape(-1, cs.C)[sl].contiguous()), t(cs.Wh), t(cs.bh), t(lab[sl].contiguous()), cs.ign,
                sums, cm, t(cs.s4))
    want = f"head_eval:{'head32' if cs.C == 32 else 'split'}{':defer' if cs.defer else ''}" if DEV == "cuda" else "cpu"
    assert o.last_path() == want
    return sums, cm


def check_counts(r, sums, cm):
    assert torch.equal(cm.cpu(), r.cm)
    assert float(sums[1]) == r.hits and float(sums[2]) == r.count
    assert int(cm.sum()) == r.count and int(cm.diag().sum()) == r.hits


@pytest.mark.parametrize("C,K,defer,P", [g + (P0,) for g in GRID] + [(32, 6, 0, PLOOP), (32, 6, 1, PLOOP)]
                         + [(32, 6, 1, PTINY), (64, 16, 1, PTINY)])
def test_exact_confusion_matrix(ops, C, K, defer, P):
    """integer logits, two identical class rows (0 and K - 1): real ties, decided by the first maximum"""
    cs, lab = inputs("tie", C, K, defer, P)
    r = reference(cs, lab)
    # (K = 2: both rows tie at every pixel, every label is 0 and only the first maximum makes a hit)
    assert int(r.cm[1].sum()) == 0 and (r.hits == r.count if K == 2 else P < 16 or 0 < r.hits < r.count < P)
    check_counts(r, *run(ops, cs, lab))


@pytest.mark.parametrize("C,K,defer", GRID)
def test_loss_gauss(ops, C, K, defer):
    cs, lab = inputs("gauss", C, K, defer, P0)
    r = reference(cs, lab)
    assert r.near == 0, f"bad case: {r.near} counted pixels within 2 eps of a tie"
    sums, cm = run(ops, cs, lab)
    check_counts(r, sums, cm)
    err = abs(float(sums[0]) - float(r.loss_px.sum()))
    print(f"loss sum error {err:.3g} bound {r.bound:.3g}")
    assert err <= r.bound


@pytest.mark.parametrize("C,K", [(32, 6), (64, 6)])
def test_accumulates_and_repeats(ops, C, K):
    cs, lab = inputs("gauss", C, K, 1, P0)
    one, two = run(ops, cs, lab), run(ops, cs, lab)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])           # two runs: the same bits
    run(ops, cs, lab, out=two)
    assert torch.equal(two[1], 2 * one[1]) and torch.equal(two[0][1:], 2 * one[0][1:])
    halves = run(ops, cs, lab, sl=slice(0, 300))
    run(ops, cs, lab, out=halves, sl=slice(300, None))
    assert torch.equal(halves[1], one[1]) and torch.equal(halves[0][1:], one[0][1:])


def _logits_path(model, x, y, k=6):
    """the stock composition on the model's logits, in fp64, and the logit bound's sum"""
    a, _ = model._engine.features(x)
    W, b = model.conv_last.weight.detach().reshape(k, -1).double(), model.conv_last.bias.detach().double()
    eps = 2.0 ** -15 * (1 + (a.double().reshape(-1, W.shape[1]).abs() @ W.abs().t() + b.abs()).max(1).values)
    z = model(x).double().movedim(1, -1).reshape(-1, k)
    top = z.topk(2, dim=1).values
    assert int((top[:, 0] - top[:, 1] <= 2 * eps).sum()) == 0, "bad case: a pixel within 2 eps of a tie"
    ce = torch.logsumexp(z, 1) - z.gather(1, y.reshape(-1, 1))[:, 0]
    cm = torch.bincount(y.reshape(-1) * k + z.argmax(1), minlength=k * k).reshape(k, k)
    return ce.sum(), cm, float(eps.sum()) + (y.numel() + 256) * 2.0 ** -24 * float(ce.abs().sum())


def test_model_evaluate_matches_logits_path():
    from ddlpc.models import UNet
    g = torch.Generator().manual_seed(5)
    x, y = torch.rand((2, 3, 32, 32), generator=g).to(DEV), torch.randint(0, 6, (2, 32, 32), generator=g).to(DEV)
    torch.manual_seed(0)
    model = UNet(out_classes=6, depth=2, width_divisor=2).to(DEV).to_hip().eval()
    with torch.no_grad():
        loss, cm, bound = _logits_path(model, x, y)
    sums, got = model.evaluate(x, y)
    assert torch.equal(got, cm) and float(sums[2]) == y.numel() and float(sums[1]) == int(cm.diag().sum())
    assert abs(float(sums[0]) - float(loss)) <= bound
    model.evaluate(x, y, out=(sums, got))
    assert torch.equal(got, 2 * cm)
    s2, c2 = model.detach_engine().evaluate(x, y)          # the stock composition: same contract
    assert int(c2.sum()) == y.numel() == int(s2[2]) and int(c2.diag().sum()) == int(s2[1])


def test_trainer_validate_fused_on_and_off():
    from ddlpc.config import ModelConfig, TrainConfig, add_config_args, config_from_args
    from ddlpc.train.trainer import Trainer
    cfg = config_from_args(add_config_args(argparse.ArgumentParser()).parse_args(["--fused-eval", "false"]))
    assert cfg.fused_eval is False and TrainConfig().fused_eval is True
    assert TrainConfig.from_dict(cfg.to_dict()).fused_eval is False
    out = []
    for fused in (True, False):
        tr = Trainer(TrainConfig(model=ModelConfig(out_classes=6, depth=2), tile=32, num_samples=6, test_holdout=4,
                                 batch_per_gpu=2, impl="hip", log_every=0, log_dir=None, fused_eval=fused).validate(),
                     device=DEV)
        out.append(tr.validate())
        x, y = tr._to_device(*tr.test_set.get(list(range(len(tr.test_set)))))
        with torch.no_grad():
            bound = _logits_path(tr.model.eval(), x, y)[2] / y.numel()
        tr.close()
    assert out[0].keys() == out[1].keys() and abs(out[0]["val_loss"] - out[1]["val_loss"]) <= bound
    assert all(out[0][key] == out[1][key] for key in ("val_pixel_acc", "val_iou", "val_miou"))
