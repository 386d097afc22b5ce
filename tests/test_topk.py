"""Top-k gradient codec with error feedback: the ``topk_encode`` / ``topk_decode_sum`` operators
(CPU kernels here, the gfx950 kernels of csrc/topk.hip on a GPU) against the torch oracle of
``parallel/codec.py``, bit for bit — floats are compared through their int32 view (NaNs occur)."""
import math

import pytest
import torch

from ddlpc.ops import codec_ops
from ddlpc.parallel import codec as C

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
SIZES = [1, 7, 256, 4097, 50001]        # smallest, scalar tail only, one workgroup step, ragged, 7 chunks
KINDS = ["ints", "lowbits", "exponents", "normal", "nonfinite", "zeros"]


def _counts(n):
    return sorted({1, math.ceil(n / 100), max(1, n // 2), n})


def _data(kind, n, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + n)
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    if kind == "ints":                  # massive ties at the threshold; zeros and -0.0
        x = torch.randint(-4, 5, (n,), generator=gen).float()
        x[(x == 0).nonzero()[::2]] = -0.0
        return x
    if kind == "lowbits":               # 1.0f + 10 random low mantissa bits: the last two digits decide
        return (torch.randint(0, 1024, (n,), generator=gen, dtype=torch.int32) | 0x3F800000).view(torch.float32) * sign
    if kind == "exponents":             # +-2^e over every finite exponent; exponent 0 holds subnormals
        ex = torch.randint(0, 255, (n,), generator=gen, dtype=torch.int32)
        mant = torch.randint(1, 1 << 23, (n,), generator=gen, dtype=torch.int32)
        return ((ex << 23) | torch.where(ex == 0, mant, torch.zeros_like(mant))).view(torch.float32) * sign
    if kind == "zeros":
        return torch.zeros(n)
    x = torch.randn(n, generator=gen) * 1e-3
    if kind == "nonfinite":
        x[0], x[n // 2], x[n - 1] = float("nan"), float("inf"), float("-inf")
    return x


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _offset(t, off, device):
    """A copy of t on device that starts ``off`` floats past an allocation's 16-byte boundary."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=device)
    buf[off:].copy_(t)
    return buf[off:]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,k", [(n, k) for n in SIZES for k in _counts(n)])
@pytest.mark.parametrize("device", DEVICES)
def test_encode_matches_oracle(device, n, k, kind):
    """Two successive calls on one residual: g, then g reversed (the second selects from a
    non-trivial residual).  The residual starts n % 4 floats past a 16-byte boundary; the first
    gradient shares that alignment (16-byte loads of both), the second does not."""
    g = _data(kind, n)
    e_ref = torch.zeros(n)
    e = _offset(e_ref, n % 4, device)
    for gi, off in ((g, n % 4), (g.flip(0), 0)):
        want_idx, want_val = C.topk_encode(gi, e_ref, k)
        idx, val = codec_ops.topk_encode(_offset(gi, off, device), e, k)
        assert idx.dtype == torch.int32 and idx.shape == (k,) and val.shape == (k,)
        assert torch.equal(idx.cpu(), want_idx)
        assert torch.equal(_bits(val), _bits(want_val))
        assert torch.equal(_bits(e), _bits(e_ref))


def _payloads(kind, n, world):
    k = n // 2 + 1                      # more than half of the entries each: every two ranks overlap
    enc = [C.topk_encode(_data(kind, n, seed=r + 1), torch.zeros(n), k) for r in range(world)]
    return [i for i, _ in enc], [v for _, v in enc]


@pytest.mark.parametrize("weights", ["mean", "reference"])
@pytest.mark.parametrize("kind", ["ints", "normal"])
@pytest.mark.parametrize("n", [1, 4097, 50001])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("device", DEVICES)
def test_decode_sum_matches_oracle(device, world, n, kind, weights):
    idx, val = _payloads(kind, n, world)
    w = [1.0 / world] * world if weights == "mean" else C.reference_weights(world)
    want = C.topk_decode_sum(torch.full((n,), float("nan")), idx, val, w)
    out = _offset(torch.full((n,), float("nan")), n % 4, device)
    codec_ops.topk_decode_sum(out, [i.to(device) for i in idx], [v.to(device) for v in val], w)
    assert torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize("device", DEVICES)
def test_decode_sum_all_indices_in_last_tile(device):
    """Every index lies in the last 4096-float tile: the earlier tiles are written as +0.0 over
    an ``out`` full of garbage, and the overlapping index takes both ranks in rank order."""
    n = 3 * 4096 + 5
    idx = [torch.tensor([n - 4, n - 1], dtype=torch.int32), torch.tensor([n - 2, n - 1], dtype=torch.int32)]
    val = [torch.tensor([1.5, 3.0e-8]), torch.tensor([-2.25, 1.0])]
    w = [1.0 / 3, 0.5]
    want = torch.zeros(n)
    want[n - 4], want[n - 2] = torch.tensor(1.5) * torch.tensor(w[0]), -2.25 * 0.5
    want[n - 1] = torch.tensor(3.0e-8) * torch.tensor(w[0]) + torch.tensor(0.5)
    assert torch.equal(_bits(C.topk_decode_sum(torch.full((n,), -7.0), idx, val, w)), _bits(want))
    out = _offset(torch.full((n,), float("nan")), 3, device)
    codec_ops.topk_decode_sum(out, [i.to(device) for i in idx], [v.to(device) for v in val], w)
    assert torch.equal(_bits(out), _bits(want))


def test_topk_config_and_cli():
    from ddlpc.config import TrainConfig, add_config_args, config_from_args
    import argparse
    with pytest.raises(ValueError):
        TrainConfig(grad_codec="topk", codec_scale="global").validate()
    with pytest.raises(ValueError):
        TrainConfig(grad_codec="topk", topk_ratio=0).validate()
    args = add_config_args(argparse.ArgumentParser()).parse_args(["--grad-codec", "topk", "--topk-ratio", "0.02"])
    cfg = config_from_args(args)
    assert cfg.grad_codec == "topk" and cfg.topk_ratio == 0.02
    assert [C.topk_count(n, 0.02) for n in (1, 49, 50, 51, 10**6)] == [1, 1, 1, 2, 20000]
