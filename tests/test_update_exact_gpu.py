"""Exact tests of the gradient codec, the Adam update and the layout kernels of ``csrc/misc.hip``
(``update_cases.py`` explains the method; docs/TESTING.md, "Gradient codec, Adam and layout
kernels", lists the cases and derives the bounds).

``test_codec_matches_oracle`` feeds the codec Gaussian data in two segments shorter than one trip
of the encode grid and compares the decode with ``allclose``; the two Adam tests compare ``p``
alone with ``allclose`` after a few steps at n = 10 007.  A kernel that rounds ties away from zero,
hides a NaN gradient, drops the second trip of a grid-stride loop or writes a moment wrongly
passes them.  Here the codec is held to the torch oracle bit for bit on a segment table with every
edge, Adam per element and per step to an fp64 reference with derived bounds, and ``weight_pack``
/ ``to_nhwc_bf16`` to written-out permutations bit for bit.

``test_update_exact_cpu.py`` runs this module on the CPU kernels (same text, DEV = "cpu"), which
also proves every precondition and reference without a GPU.
"""
import math
import time

import pytest
import torch

import update_cases as uc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    return uc.ops()


# ------------------------------------------------------------------ codec
@pytest.mark.parametrize("place", ["none", "first", "last", "negative", "outside"])
@pytest.mark.parametrize("codec", uc.CODECS)
def test_codec_segment_table(ops, codec, place):
    uc.run_table(DEV, codec, place)


@pytest.mark.parametrize("codec", uc.CODECS)
def test_codec_ties(ops, codec):
    uc.run_ties(DEV, codec)


@pytest.mark.parametrize("codec", uc.CODECS)
def test_codec_magnitudes(ops, codec):
    uc.run_magnitudes(DEV, codec)


@pytest.mark.parametrize("codec", uc.CODECS)
def test_codec_subnormal(ops, codec):
    uc.run_subnormal(DEV, codec)


DECODE = [
    # world, weights, bit-exact against the oracle (weights that are powers of two)
    pytest.param(1, [1.0], True, id="w1-one"),
    pytest.param(2, [1.0, 1.0], True, id="w2-sum"),
    pytest.param(3, uc.reference_weights(3), True, id="w3-reference"),
    pytest.param(3, [1 / 3] * 3, False, id="w3-mean"),
    pytest.param(4, uc.reference_weights(4), False, id="w4-reference"),
    pytest.param(7, [1 / 7] * 7, False, id="w7-mean"),
]


@pytest.mark.parametrize("world,weights,exact", DECODE)
@pytest.mark.parametrize("codec", uc.CODECS)
def test_codec_decode(ops, codec, world, weights, exact):
    uc.run_decode(DEV, codec, world, weights, exact)


@pytest.mark.parametrize("where", list(uc.NONFINITE_AT))
@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf], ids=["nan", "inf", "neginf"])
@pytest.mark.parametrize("codec", uc.CODECS)
def test_codec_nonfinite(ops, codec, bad, where):
    uc.run_nonfinite(DEV, codec, bad, where)


# ------------------------------------------------------------------ Adam
@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["wd0", "wd0.01"])
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 10_007])
def test_adam_step(ops, n, wd):
    uc.run_adam(ops, DEV, n, wd)


@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["wd0", "wd0.01"])
def test_adam_step_view(ops, wd):
    """a view 4 099 floats into a larger buffer (16-byte misaligned for the float4 loop)"""
    uc.run_adam(ops, DEV, 10_007, wd, offset=4099)


@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["wd0", "wd0.01"])
@pytest.mark.parametrize("n", [3, 1027, 10_007])
def test_adam_step_dev(ops, n, wd):
    uc.run_adam(ops, DEV, n, wd, dev_scal=True)


# The grid caps at 2 048 workgroups of 256 threads, a float4 each: the second trip of the loop
# starts above 2 097 152 elements.  Two full trips, a partial third and the scalar tail.  GPU only
# (the CPU kernel has no grid).
@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["wd0", "wd0.01"])
def test_adam_second_trip(ops, wd):
    n = uc.ADAM_BIG
    assert n == 2 * 2_097_152 + 3 * 1024 + 3 and (n // 4) % (2048 * 256) == 3 * 256 and n % 4 == 3
    t0 = time.perf_counter()
    uc.run_adam(ops, DEV, n, wd)
    print(f"second-trip Adam wd={wd}: {time.perf_counter() - t0:.1f} s")


# ------------------------------------------------------------------ weight_pack, to_nhwc_bf16
@pytest.mark.parametrize("max_elems", [None, 1], ids=["largest", "one-workgroup"])
def test_weight_pack(ops, max_elems):
    uc.run_weight_pack(ops, DEV, max_elems)


# (5, 4) pads to 8 channels and so runs the 8-channel kernel; (3, 1), (5, 1) and (9, 4) keep
# Cp % 8 != 0 and run the generic one
NHWC = [(3, 8, 8), (4, 8, 8), (8, 8, 8), (12, 8, 16), (3, 1, 3), (5, 4, 8), (5, 1, 5), (9, 4, 12)]


@pytest.mark.parametrize("dims", [2, 3], ids=["4d", "5d"])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C,cpad,Cp", NHWC)
def test_to_nhwc(ops, C, cpad, Cp, dtype, layout, dims):
    assert uc.run_to_nhwc(ops, DEV, C, cpad, dtype, layout, dims) == Cp


# ------------------------------------------------------------------ bindings
def test_empty_calls(ops):
    uc.run_empty(ops, DEV)


# GPU only: the checks of the GPU bindings (csrc/bindings.cpp); the CPU kernels go through torch
# operators, which make their own
@pytest.mark.parametrize("name", uc.BINDING_NAMES)
def test_binding_refuses(ops, name):
    with pytest.raises(RuntimeError):
        uc.binding_calls(ops, DEV)[name]()
    torch.cuda.synchronize()


def test_report():
    """(prints the records for docs/TESTING.md: worst error / bound per family, tie shares)"""
    for k in sorted(uc.WORST):
        print(f"worst error / bound  {k:46s} {uc.WORST[k]:.3f}")
    for k in sorted(uc.TIES):
        print(f"tie share            {k:46s} {uc.TIES[k]:.3f}")
