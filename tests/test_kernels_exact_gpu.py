"""Bit-exact integer tests of the conv, convT and weight-gradient kernels, one case per kernel
variant, and per-element bounds for the non-linear kernels.

The norm tests of ``test_kernels_gpu.py`` (relative Frobenius error < 1e-2 on Gaussian data)
pass while ~1e-4 of the output energy is wrong: several hundred garbage outputs, one missing
halo row, one pixel dropped from a masked weight-gradient tile.  Here the kernels get small
integers, for which fp32 accumulation is exact in any order, and must equal an fp64 reference
bit for bit (``exact_cases.py`` explains the method and asserts its precondition per case).

Every case names the ``torch.ops.ddlpc.last_path()`` it is written for and asserts it after
the call (GPU only; the CPU kernels report ``cpu``), so a retuned launch heuristic cannot
silently move a case onto another kernel: change the SHAPE then, never the expectation.
Small shapes reach the chip-filling variants because a module fixture pins ``num_cus()`` to 8
(``set_cu_reserve(phys - 8)``): a 9-tile problem then takes the resident / cfg 4 / cfg 5
paths and every persistent workgroup loops over several tiles.  A second group runs at
reserve 0, where the grid exceeds the work items (idle workgroups' statistics rows, split-K).

``test_kernels_exact_cpu.py`` runs this module on the CPU kernels (same text, DEV = "cpu"),
which also proves every case's precondition and reference without a GPU.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import exact_cases as xc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    return xc.ops()


@contextlib.contextmanager
def cu_reserve(o, cus):
    """run with num_cus() pinned to `cus` (0 = the whole chip); reserve 0 restored after"""
    if DEV != "cuda":
        yield
        return
    try:
        phys = int(o.set_cu_reserve(0))
        if cus:
            o.set_cu_reserve(phys - cus)
            assert int(o.set_cu_reserve(-1)) == cus
        yield
    finally:
        o.set_cu_reserve(0)


@pytest.fixture(scope="module")
def cus8(ops):
    """grids sized for 8 CUs for the whole module; the reserve-0 tests lift it for their call"""
    with cu_reserve(ops, 8):
        yield


def C(kind, path, **c):
    return pytest.param(kind, path, c, id=f"{kind}-{path}-" + "x".join(
        str(c[k]) for k in ("N", "D", "H", "W") if k in c) + "".join(
        f"-{k}{v}" for k, v in c.items() if k not in ("N", "D", "H", "W", "family")))


# ---------------------------------------------------------------------------------------------
# Cases at num_cus() == 8: (runner, last_path() the shape is written for, parameters).
# Densities: 0.5; 0.25 from 256 input channels up and wherever a prologue or 27 taps make the sums
# larger (0.125 in the two largest such cases), so every precondition holds with margin
# (exact_cases.py lists the worst figures).
CASES_8 = [
    # ---- conv3_fwd forward, resident-weight kernel (conv3x3_res.hip).  kRes entries the
    # planner can return: 1, 4, 5, 6, 7, 9 (0 / 3 / 8 are fall-backs behind an LDS limit that
    # no accepted channel count exceeds, 2 is not a candidate: docs/TESTING.md)
    C("fwd", "conv3_fwd:res:v1", N=2, H=50, W=40, C1=32, Cout=32, bias=1, pro=1),
    C("fwd", "conv3_fwd:res:v4", N=2, H=50, W=40, C1=8, Cout=32, bias=1, img=1),
    C("fwd", "conv3_fwd:res:v5", N=2, H=50, W=40, C1=64, C2=32, Cout=32, bias=1, pro=1, pro2=1, dens=0.25),
    C("fwd", "conv3_fwd:res:v6", N=2, H=40, W=24, C1=32, Cout=64, bias=1, pro=1),
    C("fwd", "conv3_fwd:res:v6", N=3, H=20, W=18, C1=64, Cout=64, bias=1),
    C("fwd", "conv3_fwd:res:v6", N=4, H=20, W=18, C1=32, Cout=64, pro=1, groups=2),
    C("fwd", "conv3_fwd:res:v9", N=2, D=3, H=20, W=40, C1=8, Cout=32, bias=1, img=1, family="conv3d_fwd"),
    # ---- conv3_fwd forward, streaming kernel (conv3x3_fwd.hip), 2-D cfg 0-5
    C("fwd", "conv3_fwd:stream:cfg0:ks1", N=2, H=20, W=18, C1=32, Cout=32, bias=1, pro=1),
    C("fwd", "conv3_fwd:stream:cfg1:ks1", N=2, H=12, W=40, C1=64, Cout=64, bias=1, pro=1),
    C("fwd", "conv3_fwd:stream:cfg2:ks1", N=2, H=23, W=40, C1=128, Cout=128, bias=1, pro=1, dens=0.25),
    C("fwd", "conv3_fwd:stream:cfg3:ks1", N=2, H=12, W=20, C1=128, Cout=128, bias=1),
    C("fwd", "conv3_fwd:stream:cfg3:ks4", N=2, H=8, W=8, C1=256, Cout=256, bias=1, pro=1, dens=0.25),
    # cfg 4: even (super-stages) and odd (2-deep ring) 32-channel chunk counts
    C("fwd", "conv3_fwd:stream:cfg4:ks1", N=2, H=30, W=30, C1=128, Cout=128, bias=1, pro=1, dens=0.25),
    C("fwd", "conv3_fwd:stream:cfg4:ks1", N=2, H=30, W=30, C1=128, C2=32, Cout=128, bias=1),
    C("fwd", "conv3_fwd:stream:cfg5:ks1", N=2, H=62, W=32, C1=128, Cout=128, bias=1, pro=1, dens=0.125),
    C("fwd", "conv3_fwd:stream:cfg5:ks1", N=2, H=62, W=32, C1=128, C2=64, Cout=256, co1=128),
    # ---- conv3_fwd as the data gradient (pk.dgrad)
    C("dgrad", "conv3_fwd:res:v7:split", N=2, H=40, W=24, Cin=96, Cout=32, co1=64),
    C("dgrad", "conv3_fwd:res:v1:split", N=2, H=50, W=40, Cin=48, Cout=32, co1=16),
    C("dgrad", "conv3_fwd:res:v1:split", N=2, H=50, W=40, Cin=160, Cout=32, co1=128),
    C("dgrad", "conv3_fwd:res:v6:split", N=2, H=40, W=24, Cin=128, Cout=32, co1=64),
    C("dgrad", "conv3_fwd:res:v1:bnb", N=2, H=50, W=40, Cin=32, Cout=32, bnb=1),
    C("dgrad", "conv3_fwd:res:v6:bnb", N=2, H=40, W=24, Cin=64, Cout=64, bnb=1),
    C("dgrad", "conv3_fwd:res:v6:bnb", N=4, H=20, W=18, Cin=64, Cout=64, bnb=1, groups=2),
    C("dgrad", "conv3_fwd:stream:cfg0:ks1:bnb", N=2, H=20, W=18, Cin=32, Cout=32, bnb=1),
    C("dgrad", "conv3_fwd:stream:cfg1:ks1:bnb", N=2, H=12, W=40, Cin=64, Cout=64, bnb=1),
    C("dgrad", "conv3_fwd:stream:cfg3:ks4:bnb", N=2, H=8, W=8, Cin=256, Cout=256, bnb=1, dens=0.25),
    C("dgrad", "conv3_fwd:stream:cfg4:ks1:bnb", N=2, H=30, W=30, Cin=128, Cout=128, bnb=1),
    C("dgrad", "conv3_fwd:stream:cfg2:ks1:bnb", N=2, H=23, W=40, Cin=128, Cout=128, bnb=1),
    C("dgrad", "conv3_fwd:stream:cfg3:ks1:bnb", N=2, H=12, W=20, Cin=128, Cout=128, bnb=1),
    C("dgrad", "conv3_fwd:stream:cfg1:ks1", N=2, H=12, W=40, Cin=64, Cout=32, co1=32),
    # ---- 3-D forward: depth-streaming kernel, the 4-wave and 8-wave streaming configurations
    C("fwd", "conv3_fwd:ds", N=2, D=5, H=20, W=18, C1=32, Cout=64, co1=32, pro=1, dens=0.25, family="conv3d_fwd"),
    C("fwd", "conv3_fwd:ds", N=2, D=3, H=20, W=18, C1=32, Cout=32, bias=1, family="conv3d_fwd"),
    C("fwd", "conv3_fwd:stream3d:cfg0:ks1", N=2, D=5, H=8, W=8, C1=64, Cout=32, bias=1, pro=1, dens=0.25, family="conv3d_fwd"),
    C("fwd", "conv3_fwd:stream3d:cfg1:ks1", N=2, D=5, H=8, W=8, C1=64, Cout=64, bias=1, family="conv3d_fwd"),
    C("fwd", "conv3_fwd:stream3d:cfg2:ks1", N=2, D=7, H=16, W=8, C1=64, Cout=128, bias=1, family="conv3d_fwd"),
    C("fwd", "conv3_fwd:stream3d:cfg3:ks1", N=2, D=5, H=8, W=8, C1=64, Cout=128, bias=1, pro=1, dens=0.25, family="conv3d_fwd"),
    C("fwd", "conv3_fwd:stream3d:cfg6:ks1", N=2, D=11, H=8, W=16, C1=64, Cout=32, bias=1, pro=1, dens=0.125, family="conv3d_fwd"),
    C("fwd", "conv3_fwd:stream3d:cfg7:ks1", N=2, D=7, H=8, W=16, C1=64, Cout=64, bias=1, family="conv3d_fwd"),
    C("fwd", "conv3_fwd:stream3d:cfg8:ks1", N=2, D=7, H=4, W=16, C1=64, Cout=128, bias=1, pro=1, dens=0.25, family="conv3d_fwd"),
    C("dgrad", "conv3_fwd:stream3d:cfg9:ks1", N=2, D=7, H=8, W=16, Cin=96, Cout=64, co1=64, family="conv3d_fwd"),
    # ---- conv3_wgrad: every branch of the launch chain
    C("wgrad", "conv3_wgrad:v1", N=2, H=10, W=6, C1=32, Cout=32, pro=1),
    C("wgrad", "conv3_wgrad:v2", N=2, H=20, W=18, C1=16, Cout=64, pro=1),
    C("wgrad", "conv3_wgrad:v2", N=2, H=20, W=18, C1=32, C2=16, Cout=32, pro=1, pro2=1),
    C("wgrad", "conv3_wgrad:v2:dypro", N=2, H=20, W=18, C1=8, Cout=32, dypro=1),
    C("wgrad", "conv3_wgrad:img", N=2, H=20, W=18, C1=8, Cout=32, img=1),
    C("wgrad", "conv3_wgrad:img", N=3, H=40, W=24, C1=8, Cout=64, img=1),
    C("wgrad", "conv3_wgrad:img:dypro", N=2, H=20, W=18, C1=8, Cout=32, img=1, dypro=1),
    C("wgrad", "conv3_wgrad:v3:bco32:ciw1", N=2, H=20, W=18, C1=32, Cout=32, pro=1),
    C("wgrad", "conv3_wgrad:v3:bco32:ciw1", N=4, H=20, W=18, C1=32, Cout=32, pro=1, groups=2),
    C("wgrad", "conv3_wgrad:v3:bco64:ciw1", N=2, H=20, W=18, C1=64, C2=32, Cout=64, pro=1, pro2=1),
    C("wgrad", "conv3_wgrad:v3:bco64:ciw2", N=2, H=72, W=58, C1=64, Cout=64, pro=1),
    C("wgrad", "conv3_wgrad:v3:bco128:ciw1", N=2, H=36, W=30, C1=32, Cout=128, pro=1),
    C("wgrad", "conv3_wgrad:c32", N=2, H=72, W=100, C1=64, C2=32, Cout=32, pro=1, pro2=1),
    C("wgrad", "conv3_wgrad:c32", N=2, H=72, W=100, C1=32, C2=32, Cout=32),
    C("wgrad", "conv3_wgrad:c32:dyout", N=2, H=72, W=100, C1=64, C2=32, Cout=32, dypro=1, dyout=1),
    # ---- 3-D weight gradients
    C("wgrad", "conv3_wgrad:ds", N=2, D=5, H=72, W=58, C1=32, Cout=32, pro=1, family="conv3d_wgrad"),
    C("wgrad", "conv3_wgrad:img:3d", N=2, D=5, H=20, W=18, C1=8, Cout=32, img=1, family="conv3d_wgrad"),
    C("wgrad", "conv3_wgrad:v3:bco64:ciw1:3d", N=2, D=5, H=12, W=20, C1=32, Cout=64, pro=1, family="conv3d_wgrad"),
    C("wgrad", "conv3_wgrad:v3:bco32:ciw1:3d", N=2, D=5, H=12, W=20, C1=32, Cout=32, family="conv3d_wgrad"),
    C("wgrad", "conv3_wgrad:v3:bco128:ciw1:3d", N=2, D=3, H=36, W=30, C1=32, Cout=128, family="conv3d_wgrad"),
    C("wgrad", "conv3_wgrad:v2:3d", N=2, D=3, H=12, W=20, C1=16, Cout=32, family="conv3d_wgrad"),
    C("wgrad", "conv3_wgrad:v1:3d", N=2, D=3, H=10, W=6, C1=32, Cout=32, family="conv3d_wgrad"),
    # ---- the fused 32-channel backward
    C("bwd32", "conv3_bwd32", N=2, H=50, W=18),
    C("bwd32", "conv3_bwd32", N=3, H=40, W=24),
    C("bwd32", "conv3_bwd32:groups", N=4, H=20, W=18, groups=2),
    # ---- transposed conv: both back ends of the forward and the data gradient, both
    # weight-gradient kernels, the fused backward
    C("convt_fwd", "convt_fwd:res", N=2, H=12, W=20, Cin=64, Cout=64, bn=1),
    C("convt_fwd", "convt_fwd:res", N=2, H=12, W=20, Cin=128, Cout=64),
    C("convt_fwd", "convt_fwd:gemm", N=2, H=6, W=10, Cin=512, Cout=256, bn=1, dens=0.25),
    C("convt_fwd", "convt_fwd:gemm", N=3, H=6, W=10, Cin=40, Cout=24),
    C("convt_dgrad", "convt_dgrad:res", N=2, H=12, W=20, Cin=64, Cout=64, bn=1),
    C("convt_dgrad", "convt_dgrad:res", N=3, H=6, W=10, Cin=64, Cout=32),
    C("convt_dgrad", "convt_dgrad:gemm", N=2, H=12, W=20, Cin=128, Cout=64),
    C("convt_dgrad", "convt_dgrad:gemm", N=2, H=6, W=10, Cin=512, Cout=256, bn=1),
    C("convt_dgrad", "convt_dgrad:gemm", N=3, H=6, W=10, Cin=96, Cout=64, bn=1),
    C("convt_wgrad", "convt_wgrad:wg2", N=2, H=12, W=20, Cin=64, Cout=64, bn=1),
    C("convt_wgrad", "convt_wgrad:wg2", N=3, H=6, W=10, Cin=128, Cout=64),
    C("convt_wgrad", "convt_wgrad:wg1", N=2, H=6, W=10, Cin=1024, Cout=64, dens=0.25),
    C("convt_bwd_fused", "convt_bwd_fused:fused", N=3, H=12, W=20, Cin=64, Cout=64, bn=1),
    C("convt_bwd_fused", "convt_bwd_fused:fused", N=2, H=6, W=10, Cin=64, Cout=64),
    C("convt_bwd_fused", "convt_bwd_fused:separate", N=2, H=6, W=10, Cin=128, Cout=64, bn=1),
    # 3-D transposed conv
    C("convt_fwd", "convt_fwd:res", N=2, D=2, H=6, W=10, Cin=64, Cout=64, bn=1),
    C("convt_dgrad", "convt_dgrad:gemm", N=2, D=2, H=6, W=10, Cin=64, Cout=64, bn=1),
    C("convt_wgrad", "convt_wgrad:wg2", N=2, D=2, H=6, W=10, Cin=64, Cout=64),
]

# Cases at reserve 0 (the whole chip): more workgroups than work items — split-K over the input
# channel chunks (needs items < num_cus) and idle workgroups' statistics rows
CASES_0 = [
    C("fwd", "conv3_fwd:stream:cfg0:ks2", N=2, H=20, W=18, C1=128, Cout=32, bias=1, pro=1, dens=0.25),
    C("fwd", "conv3_fwd:stream:cfg1:ks2", N=2, H=20, W=18, C1=128, Cout=64, bias=1),
    C("fwd", "conv3_fwd:stream:cfg3:ks4", N=2, H=8, W=8, C1=256, Cout=256, bias=1, pro=1, dens=0.25),
    C("fwd", "conv3_fwd:stream:cfg0:ks1", N=2, H=20, W=18, C1=32, Cout=32, bias=1, pro=1),
    C("dgrad", "conv3_fwd:stream:cfg1:ks2:bnb", N=2, H=20, W=18, Cin=64, Cout=128, bnb=1),
    C("fwd", "conv3_fwd:stream3d:cfg0:ks2", N=2, D=5, H=8, W=8, C1=128, Cout=32, bias=1, dens=0.25, family="conv3d_fwd"),
    C("fwd", "conv3_fwd:stream3d:cfg1:ks2", N=2, D=5, H=8, W=8, C1=128, Cout=64, bias=1, dens=0.25, family="conv3d_fwd"),
    C("fwd", "conv3_fwd:stream3d:cfg3:ks2", N=2, D=5, H=8, W=8, C1=128, Cout=128, bias=1, dens=0.25, family="conv3d_fwd"),
    C("wgrad", "conv3_wgrad:v3:bco32:ciw1", N=2, H=20, W=18, C1=32, Cout=32, pro=1),
    C("bwd32", "conv3_bwd32", N=2, H=20, W=18),
    C("convt_dgrad", "convt_dgrad:res", N=2, H=12, W=20, Cin=64, Cout=64, bn=1),
    C("convt_bwd_fused", "convt_bwd_fused:fused", N=2, H=6, W=10, Cin=64, Cout=64, bn=1),
]

# The coverage condition: every dispatch path that must have a case (test_paths_covered).
PATHS = [
    # conv3_fwd_launch: every reachable (configuration, split-K) pair.  Split-K needs fewer
    # work items than CUs, which cfg 2 / 4 / 5 / 6-9 exclude by their fill conditions.
    "conv3_fwd:stream:cfg0:ks1", "conv3_fwd:stream:cfg1:ks1", "conv3_fwd:stream:cfg2:ks1",
    "conv3_fwd:stream:cfg3:ks1", "conv3_fwd:stream:cfg4:ks1", "conv3_fwd:stream:cfg5:ks1",
    "conv3_fwd:stream:cfg0:ks2", "conv3_fwd:stream:cfg1:ks2", "conv3_fwd:stream:cfg3:ks4",
    "conv3_fwd:stream3d:cfg0:ks1", "conv3_fwd:stream3d:cfg1:ks1", "conv3_fwd:stream3d:cfg2:ks1",
    "conv3_fwd:stream3d:cfg3:ks1", "conv3_fwd:stream3d:cfg6:ks1", "conv3_fwd:stream3d:cfg7:ks1",
    "conv3_fwd:stream3d:cfg8:ks1", "conv3_fwd:stream3d:cfg9:ks1",
    "conv3_fwd:stream3d:cfg0:ks2", "conv3_fwd:stream3d:cfg1:ks2", "conv3_fwd:stream3d:cfg3:ks2",
    # the BN-backward epilogue variants of the streaming kernel and of the split-K finalize
    "conv3_fwd:stream:cfg0:ks1:bnb", "conv3_fwd:stream:cfg1:ks1:bnb", "conv3_fwd:stream:cfg4:ks1:bnb",
    "conv3_fwd:stream:cfg2:ks1:bnb", "conv3_fwd:stream:cfg3:ks1:bnb",
    "conv3_fwd:stream:cfg3:ks4:bnb", "conv3_fwd:stream:cfg1:ks2:bnb",
    # conv3_res_plan: every kRes entry it can return, with the split store and the BN-backward
    # epilogue where the variant has them
    "conv3_fwd:res:v1", "conv3_fwd:res:v4", "conv3_fwd:res:v5", "conv3_fwd:res:v6", "conv3_fwd:res:v9",
    "conv3_fwd:res:v7:split", "conv3_fwd:res:v1:split", "conv3_fwd:res:v6:split", "conv3_fwd:res:v1:bnb", "conv3_fwd:res:v6:bnb",
    # the depth-streaming kernels
    "conv3_fwd:ds", "conv3_wgrad:ds",
    # conv3_wgrad's launch chain
    "conv3_wgrad:c32", "conv3_wgrad:c32:dyout", "conv3_wgrad:img", "conv3_wgrad:img:dypro",
    "conv3_wgrad:img:3d", "conv3_wgrad:v3:bco32:ciw1", "conv3_wgrad:v3:bco64:ciw1",
    "conv3_wgrad:v3:bco64:ciw2", "conv3_wgrad:v3:bco128:ciw1", "conv3_wgrad:v3:bco64:ciw1:3d",
    "conv3_wgrad:v3:bco32:ciw1:3d", "conv3_wgrad:v3:bco128:ciw1:3d",
    "conv3_wgrad:v2", "conv3_wgrad:v2:dypro", "conv3_wgrad:v2:3d", "conv3_wgrad:v1", "conv3_wgrad:v1:3d",
    "conv3_bwd32", "conv3_bwd32:groups",
    # transposed conv
    "convt_fwd:res", "convt_fwd:gemm", "convt_dgrad:res", "convt_dgrad:gemm",
    "convt_wgrad:wg2", "convt_wgrad:wg1", "convt_bwd_fused:fused", "convt_bwd_fused:separate",
]


def _run(ops, kind, path, c):
    got = xc.run_case(ops, DEV, kind, c)
    if DEV == "cuda":
        assert got == path, f"shape dispatched to {got!r}, written for {path!r}: change the shape"
    else:
        assert got == "cpu"


@pytest.mark.parametrize("kind,path,c", CASES_8)
def test_exact(ops, cus8, kind, path, c):
    _run(ops, kind, path, c)


@pytest.mark.parametrize("kind,path,c", CASES_0)
def test_exact_whole_chip(ops, cus8, kind, path, c):
    try:
        with cu_reserve(ops, 0):
            _run(ops, kind, path, c)
    finally:
        if DEV == "cuda":                   # back to the module's 8 CUs, pass or fail
            ops.set_cu_reserve(int(ops.set_cu_reserve(0)) - 8)
            assert int(ops.set_cu_reserve(-1)) == 8


def test_paths_covered():
    """every listed dispatch path has a case that asserts it (and no case names an unlisted
    path, so the list stays the module's table of contents)"""
    asserted = {p.values[1] for p in CASES_8 + CASES_0}
    assert sorted(set(PATHS) - asserted) == [], "paths without a case"
    assert sorted(asserted - set(PATHS)) == [], "cases whose path is not listed"
    assert len(PATHS) == len(set(PATHS))


# ---------------------------------------------------------------------------------------------
# Non-linear kernels: per-element bounds |got - ref64| <= 2^-8 |ref64| + 2^-20 S instead of the
# norm (xc.assert_bound); ragged shapes, N >= 2.
def _randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).bfloat16()


@pytest.mark.parametrize("shape", [(2, 9, 7, 16), (3, 5, 12, 8), (2, 3, 5, 6, 8), (2, 4, 3, 7, 16)])
def test_bilinear_up2_elementwise(ops, cus8, shape):
    x = _randn(shape, 41)
    xr = xc.cf(x).requires_grad_(True)
    ref = xc.up2_ref(xr)
    y = ops.bilinear_up2(x.to(DEV))
    xc.assert_bound(y, xc.cl(ref.detach()), xc.cl(xc.up2_ref(xc.cf(x).abs())), "bilinear_up2")
    dy = _randn(tuple(xc.cl(ref.detach()).shape), 42)
    (gx,) = torch.autograd.grad(ref, xr, xc.cf(dy))
    xa = xc.cf(x).requires_grad_(True)
    (gs,) = torch.autograd.grad(xc.up2_ref(xa), xa, xc.cf(dy).abs())
    dx = ops.bilinear_up2_bwd(dy.to(DEV))
    xc.assert_bound(dx, xc.cl(gx), xc.cl(gs), "bilinear_up2_bwd")


def _gauss_s4(Cn, seed):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(Cn, generator=g) * 0.2
    invstd = torch.rand(Cn, generator=g) + 0.5
    scale = torch.randn(Cn, generator=g)               # negative channels included
    shift = torch.randn(Cn, generator=g) * 0.3
    return torch.stack([mean, invstd, scale, shift]).contiguous()


@pytest.mark.parametrize("shape,pool,full", [
    ((2, 9, 7, 16), False, True), ((3, 10, 6, 24), True, True), ((2, 6, 14, 8), True, False),
    ((2, 3, 5, 7, 8), False, True), ((2, 4, 6, 2, 16), True, True), ((2, 2, 6, 10, 8), True, False)])
def test_bn_relu_apply_elementwise(ops, cus8, shape, pool, full):
    y = _randn(shape, 43, 2.0, 0.5)
    s4 = _gauss_s4(shape[-1], 44)
    a, p = ops.bn_relu_apply(y.to(DEV), s4.to(DEV), pool, full)
    ref = torch.relu(y.double() * s4[2].double() + s4[3].double())
    S = y.double().abs() * s4[2].double().abs() + s4[3].double().abs()
    if full:
        xc.assert_bound(a, ref, S, "bn_relu_apply")
    else:
        assert a.numel() == 0
    if pool:
        mp = F.max_pool2d if len(shape) == 4 else F.max_pool3d
        xc.assert_bound(p, xc.cl(mp(xc.cf(ref), 2)), xc.cl(mp(xc.cf(S), 2)), "bn_relu_apply pooled")


@pytest.mark.parametrize("shape", [(2, 9, 7, 16), (3, 10, 22, 8), (2, 3, 5, 7, 8)])
def test_bn_backward_dy_elementwise(ops, cus8, shape):
    """dY = k (dyh - m1 - xhat m2) of bn_backward, k = gamma invstd, m1 / m2 the batch means of
    dyh and dyh xhat: fp64 reference of the whole formula, reductions included"""
    Cn = shape[-1]
    y, dA = _randn(shape, 45, 1.3, 0.2), _randn(shape, 46)
    s4 = _gauss_s4(Cn, 47)
    gamma = torch.rand(Cn, generator=torch.Generator().manual_seed(48)) + 0.5
    dY, dg, db = ops.bn_backward(dA.to(DEV), None, y.to(DEV), s4.to(DEV), gamma.to(DEV), None)
    dyh, xh = xc.bnb_terms(dA.double(), y, s4)
    cnt = y[..., 0].numel()
    k = gamma.double() * s4[1].double()
    m1 = dyh.reshape(-1, Cn).sum(0) / cnt
    m2 = (dyh * xh).reshape(-1, Cn).sum(0) / cnt
    ref = k * (dyh - m1 - xh * m2)
    xa = (y.double().abs() + s4[0].double().abs()) * s4[1].double()
    M1 = dyh.abs().reshape(-1, Cn).sum(0) / cnt
    M2 = (dyh.abs() * xa).reshape(-1, Cn).sum(0) / cnt
    S = k.abs() * (dyh.abs() + M1 + xa * M2)
    xc.assert_bound(dY, ref, S, "bn_backward dY")
