"""``grad_codec="powersgd"``: rank bounds, rejected combinations, CLI flags, the default model's plan."""
import argparse

import pytest
import torch
from ddlpc.config import TrainConfig, add_config_args, config_from_args
from ddlpc.parallel import codec as C
from ddlpc.parallel.flat import FlatParams


@pytest.mark.parametrize("bad", [dict(powersgd_rank=0), dict(powersgd_rank=17), dict(codec_scale="global"),
                                 dict(codec_scale="tensor"), dict(wire_dtype="bf16"), dict(comm_proxy=2)])
def test_config_rejects(bad):
    from ddlpc.parallel.reducer import GradBucketReducer
    TrainConfig(grad_codec="powersgd", powersgd_rank=16).validate()
    with pytest.raises(ValueError):
        TrainConfig(**{"grad_codec": "powersgd", **bad}).validate()
    if "comm_proxy" not in bad:           # the reducer refuses the same on its own
        with pytest.raises(ValueError):
            GradBucketReducer(FlatParams([torch.nn.Parameter(torch.zeros(8, 8))]), grad_codec="powersgd", **bad)


def test_cli_flags_reach_the_config():
    cfg = config_from_args(add_config_args(argparse.ArgumentParser()).parse_args(
        ["--grad-codec", "powersgd", "--powersgd-rank", "8"]))
    assert cfg.grad_codec == "powersgd" and cfg.powersgd_rank == 8 and TrainConfig().powersgd_rank == 4


def test_plan_of_the_default_model():
    from ddlpc.models.unet import UNet
    model = UNet.from_config(TrainConfig().model)
    flat = FlatParams([p for p in model.parameters() if p.requires_grad])
    plan = C.powersgd_plan(flat, flat.order, 0, 4)
    low, raw = {int(r[0]): (int(r[1]), int(r[2])) for r in plan.low}, {int(r[0]) for r in plan.raw}
    for name, p in model.named_parameters():
        a = flat.span(p)[0]
        if p.dim() == 1:
            assert a in raw, name
        elif p.dim() == 4 and p.shape[2] > 1:            # conv (OIHW) and transposed-conv (IOHW) weights
            assert low[a] == (p.shape[0], p.numel() // p.shape[0]), name
    assert plan.dense == sum(p.numel() for p in flat.order) > 8 * (plan.wire_p + plan.wire_q)
    assert C.powersgd_init_q(plan, 3, 1).equal(C.powersgd_init_q(plan, 3, 1))
    assert not C.powersgd_init_q(plan, 3, 1).equal(C.powersgd_init_q(plan, 3, 2))
