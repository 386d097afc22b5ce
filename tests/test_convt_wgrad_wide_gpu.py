"""Bit-exact tests of the transposed-conv weight gradient's 256-column-tile kernel
(``gemm_tn_wgrad2w_kernel``, ``last_path() == "convt_wgrad:wg2w"``).

The launch rule gives the wide kernel only chip-filling shapes, so the knob
``CONVT_WGRAD_WIDE=1`` (wherever the shape constraints hold) brings it to shapes of a few
hundred pixels.  Operands are the integer-valued ones of ``exact_cases.py`` (ternary x and dOut,
power-of-two BatchNorm scales): fp32 accumulation is exact in any order, so

* dW and db of the wide kernel equal the fp64 reference bit for bit, and
* the wide (knob 1) and the 128-column (knob 0) kernels equal each other bit for bit,
  although they split the pixels differently.

Shapes (whole chip, ``num_cus() == 256``; a stage is 32 pixels, the ring has 4 slots):

    Cin 256, Cout  64, 2x12x20   one n tile, 256 x 256 tile, 15 whole stages in one split
    Cin 256, Cout 128, 3x6x10    two n tiles; 180 px: a last stage of 20 pixels
    Cin 128, Cout  64, 2x12x20   the 128-row form (waves of 64 x 64)
    Cin 384, Cout  64, 2x6x10    an M tail of half a tile (rows 384..511 masked)
    Cin 512, Cout 128, 1x8x8     2 m tiles x 2 n tiles; splits capped by K / 256; 2 stages
                                 (fewer than ring slots)
    Cin 256, Cout  64, 2x20x26   the carry walker: W = 26 < 32, so every stage crosses an image
                                 row, and the stage at pixel 512 crosses the image boundary at
                                 520; 4 splits of 320 / 320 / 320 / 80 pixels: the last one has
                                 3 stages (fewer than ring slots), the third of 16 pixels

each with and without the deferred BatchNorm + ReLU of x (``bn4``).
"""
import pytest
import torch

import exact_cases as xc

pytestmark = pytest.mark.gpu

DEV = "cuda"
KNOB = "CONVT_WGRAD_WIDE"
CLEAR = -2 ** 63              # set_knob: drop the override

SHAPES = [
    dict(N=2, H=12, W=20, Cin=256, Cout=64, dens=0.25),
    dict(N=3, H=6, W=10, Cin=256, Cout=128, dens=0.25),
    dict(N=2, H=12, W=20, Cin=128, Cout=64),
    dict(N=2, H=6, W=10, Cin=384, Cout=64, dens=0.25),
    dict(N=1, H=8, W=8, Cin=512, Cout=128, dens=0.25),
    dict(N=2, H=20, W=26, Cin=256, Cout=64, dens=0.25),
]
CASES = [pytest.param(dict(s, bn=bn), id="x".join(str(s[k]) for k in ("N", "H", "W"))
                      + f"-Cin{s['Cin']}-Cout{s['Cout']}-bn{bn}") for s in SHAPES for bn in (0, 1)]


@pytest.fixture(scope="module")
def ops():
    o = xc.ops()
    o.set_cu_reserve(0)                     # the whole chip, whatever an earlier module left
    return o


def _wgrad(o, wide, x, dout, bn4):
    """(dW, db, last_path) with CONVT_WGRAD_WIDE = wide; the knob restored in the finally"""
    prev = int(o.set_knob(KNOB, wide))
    try:
        dW, db = o.convt_wgrad(x, dout, None, None, None, bn4)
        path = o.last_path()
        torch.cuda.synchronize()
    finally:
        o.set_knob(KNOB, prev)              # (CLEAR when it was unset)
    return dW, db, path


@pytest.mark.parametrize("c", CASES)
def test_wide_exact_and_equal_to_narrow(ops, c):
    sp, dims, x, w, dout, bn4, a, q = xc._convt_case(c)
    _, _, gw = xc._convt_refs(a, w, dout, dims)          # fp64 reference, computed once
    xd, dd = x.to(DEV), dout.to(DEV)
    bd = None if bn4 is None else bn4.to(DEV)
    dW1, db1, p1 = _wgrad(ops, 1, xd, dd, bd)
    assert p1 == "convt_wgrad:wg2w", f"knob 1 dispatched to {p1!r}"
    xc._assert_convt_grads(dW1, db1, gw, dout, a, q, "convt_wgrad")
    dW0, db0, p0 = _wgrad(ops, 0, xd, dd, bd)
    assert p0 == "convt_wgrad:wg2", f"knob 0 dispatched to {p0!r}"
    assert torch.equal(dW1, dW0), f"{int((dW1 != dW0).sum())} dW elements differ between the kernels"
    assert torch.equal(db1, db0)


def test_knob_restored_and_rule_keeps_small_shapes_narrow(ops):
    """after the cases above the knob is back to unset, and the shape rule leaves a shape of a
    few hundred pixels on the 128-column kernel"""
    prev = int(ops.set_knob(KNOB, CLEAR))
    # (-1: the default a kernel launch cached before the first override)
    assert prev in (CLEAR, -1), f"{KNOB} left at {prev}"
    sp, dims, x, w, dout, bn4, a, q = xc._convt_case(dict(SHAPES[0], bn=0))
    ops.convt_wgrad(x.to(DEV), dout.to(DEV), None, None, None, None)
    assert ops.last_path() == "convt_wgrad:wg2"
