"""Exact tests of the gradient tail (``tail_cases.py`` explains the method; docs/TESTING.md, "The
gradient tail", has the regime table, the defect table and what is not covered).

Every parameter gradient leaves the library through ``sum_slab`` -> ``reduce_rows_scatter_launch``
(fp64 row sums in a fixed order, the permutation to OIHW / IOHW, one rounding to fp32, write or
accumulate) or one of its siblings.  The exact operator suites reach only its first row-count
regime and never the accumulate branch; the direct-grad forms the training step uses were held to
``allclose`` on Gaussian data.  Here the scatter is driven as an operator through every regime
(R <= 64, <= 1 024, above) x every layout mode x a row stride, ``reduce_rows`` through its
multi-level loop, and every operator's direct-grad form must equal ``prefill + 2 dW`` bit for bit
on the integer operands whose returned gradient the exact suites prove.  No tolerance anywhere in
this module.

``test_tail_exact_cpu.py`` runs this module on the CPU kernels (same text, DEV = "cpu"), which also
proves every precondition and reference without a GPU.
"""
import contextlib

import pytest
import torch

import exact_cases as xc
import tail_cases as tc

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
    """grids sized for 8 CUs for the whole module; the whole-chip tests lift it for their call"""
    with cu_reserve(ops, 8):
        yield


@contextlib.contextmanager
def whole_chip(o):
    try:
        with cu_reserve(o, 0):
            yield
    finally:
        if DEV == "cuda":                   # back to the module's 8 CUs, pass or fail
            o.set_cu_reserve(int(o.set_cu_reserve(0)) - 8)
            assert int(o.set_cu_reserve(-1)) == 8


def _path(got, want):
    if DEV == "cuda":
        assert got == want, f"shape dispatched to {got!r}, written for {want!r}: change the shape"
    else:
        assert got == "cpu"


# ------------------------------------------------------------------ the scatter, kernel by kernel
# R: 1, 2, 64 the one-pass form and its last row count; 65 the first wide one (waves 1..3 sum 16
# rows, wave 0 17); 257 = 4 * 64 + 1; 1 024 the last wide one; 1 025 the first two-pass one (17
# chunks, the last of one row); 4 097 (reduce_rows) enters the multi-level loop: 65 chunks, then 2
ROWS = [1, 2, 64, 65, 257, 1024, 1025]
SCATTER = []
for _R in ROWS:                             # identity: the edges of the 64- and 256-column blocks
    for _N in (1, 63, 64, 65, 255, 257):
        SCATTER.append(dict(R=_R, N=_N, mode=2))
for _R in (2, 65, 1025):                    # every regime meets every layout
    for _A, _T, _B in ((5, 9, 8), (3, 27, 8), (32, 9, 32)):
        SCATTER.append(dict(R=_R, N=_A * _T * _B, mode=0, A=_A, T=_T, B=_B))
    for _A, _T, _B in ((6, 4, 10), (6, 8, 10), (64, 4, 64)):
        SCATTER.append(dict(R=_R, N=_A * _T * _B, mode=1, A=_A, T=_T, B=_B))
for _R in (8, 65, 1025):                    # rows of a [R][2][96] slab
    for _N in (24, 64):
        SCATTER.append(dict(R=_R, N=_N, mode=2, ld=192))


def _sid(c):
    return f"R{c['R']}-N{c['N']}-mode{c['mode']}" + (f"-{c['A']}x{c['T']}x{c['B']}" if c["mode"] != 2 else "") + (
        f"-ld{c['ld']}" if "ld" in c else "")


def test_scatter_cases():
    """the case list holds what it is written for"""
    small = [c["N"] for c in SCATTER if c["mode"] != 2 and c["N"] < 1000]
    assert len(small) == 12 and all(n % 64 != 0 for n in small)
    for mode in (0, 1, 2):
        assert {c["R"] for c in SCATTER if c["mode"] == mode and "ld" not in c} >= {2, 65, 1025}
    assert len(SCATTER) == 42 + 18 + 6


@pytest.mark.parametrize("c", SCATTER, ids=_sid)
def test_scatter_exact(ops, c):
    tc.run_scatter(ops, DEV, c)


REDUCE = [(R, N) for R in ROWS + [4097] for N in (1, 70, 257)] + [(300, 9216)]


@pytest.mark.parametrize("R,N", REDUCE)
def test_reduce_rows_exact(ops, R, N):
    tc.run_reduce_rows(ops, DEV, R, N)


def test_scatter_empty(ops):
    """R == 0 or N == 0: nothing is launched, the destination keeps its values"""
    buf, dst = tc.guarded(6, DEV, tc.SENT)
    ops.reduce_rows_scatter(torch.zeros(0, device=DEV), 0, 6, dst, 2, 0, 0, False, -1)
    ops.reduce_rows_scatter(torch.zeros(0, device=DEV), 0, 6, dst, 0, 3, 2, True, -1)
    assert bool((dst == tc.SENT).all())
    ops.reduce_rows_scatter(torch.zeros(4, device=DEV), 4, 0, dst[:0], 2, 0, 0, False, -1)
    tc.guards_intact(buf, 6, "empty calls")


# ------------------------------------------------------------------ direct grads
def D(kind, path, **c):
    return pytest.param(kind, path, c, id=f"{kind}-{path}-" + "x".join(
        str(c[k]) for k in ("N", "D", "H", "W") if k in c) + "".join(
        f"-{k}{v}" for k, v in c.items() if k not in ("N", "D", "H", "W", "family")))


# the operands and shapes of test_kernels_exact_gpu.py (CASES_8), one per kernel family
DIRECT = [
    D("wgrad", "conv3_wgrad:v1", N=2, H=10, W=6, C1=32, Cout=32, pro=1),
    D("wgrad", "conv3_wgrad:v2", N=2, H=20, W=18, C1=16, Cout=64, pro=1),
    D("wgrad", "conv3_wgrad:img", N=2, H=20, W=18, C1=8, Cout=32, img=1),
    D("wgrad", "conv3_wgrad:v3:bco32:ciw1", N=2, H=20, W=18, C1=32, Cout=32, pro=1),
    D("wgrad", "conv3_wgrad:v3:bco32:ciw1", N=4, H=20, W=18, C1=32, Cout=32, pro=1, groups=2),
    D("wgrad", "conv3_wgrad:c32", N=2, H=72, W=100, C1=32, C2=32, Cout=32),
    D("wgrad", "conv3_wgrad:v3:bco32:ciw1:3d", N=2, D=5, H=12, W=20, C1=32, Cout=32, family="conv3d_wgrad"),
    D("bwd32", "conv3_bwd32", N=2, H=50, W=18),
    D("bwd32", "conv3_bwd32:groups", N=4, H=20, W=18, groups=2),
    D("convt_wgrad", "convt_wgrad:wg2", N=2, H=12, W=20, Cin=64, Cout=64, bn=1),
    D("convt_wgrad", "convt_wgrad:wg1", N=2, H=6, W=10, Cin=1024, Cout=64, dens=0.25),
    D("convt_wgrad", "convt_wgrad:wg2", N=2, D=2, H=6, W=10, Cin=64, Cout=64),
    D("convt_bwd_fused", "convt_bwd_fused:fused", N=3, H=12, W=20, Cin=64, Cout=64, bn=1),
    D("convt_bwd_fused", "convt_bwd_fused:separate", N=2, H=6, W=10, Cin=128, Cout=64, bn=1),
]


def _direct(ops, kind, c):
    if kind == "wgrad":
        return tc.run_direct_conv3_wgrad(ops, DEV, c), None
    if kind == "bwd32":
        return tc.run_direct_bwd32(ops, DEV, c)
    return tc.run_direct_convt(ops, DEV, c, kind == "convt_bwd_fused"), None


@pytest.mark.parametrize("kind,path,c", DIRECT)
def test_direct_grads(ops, cus8, kind, path, c):
    _path(_direct(ops, kind, c)[0], path)


# The whole chip: conv3_bwd32 has one slab row per workgroup, min(tiles, CUs) of them
# (conv3_bwd32_grid) = 2 x 5 x 7 = 70 here, the count of BN partial rows it returns: the wide
# regime (64 < R <= 1 024) under a real operator.  The concat weight-gradient kernel (c32, one row
# per CU) needs 8 tiles per CU (conv3_wgrad_c32_plan), 2 048 tiles on 256 CUs: at this shape
# the whole chip takes the v3 kernel with min(ceil(3 CUs / 2 chunks), 70 tiles / 8) = 8 rows
# (conv3_wgrad_plan), restated here; c32's own row count is the 8 CUs of DIRECT above.
DIRECT_0 = [
    D("bwd32", "conv3_bwd32", N=2, H=72, W=100),
    D("wgrad", "conv3_wgrad:v3:bco32:ciw1", N=2, H=72, W=100, C1=32, C2=32, Cout=32),
    D("convt_bwd_fused", "convt_bwd_fused:fused", N=2, H=6, W=10, Cin=64, Cout=64, bn=1),
]


@pytest.mark.parametrize("kind,path,c", DIRECT_0)
def test_direct_grads_whole_chip(ops, cus8, kind, path, c):
    with whole_chip(ops):
        got, rows = _direct(ops, kind, c)
        _path(got, path)
        if DEV == "cuda":
            cus = int(ops.set_cu_reserve(-1))
            if kind == "bwd32":
                assert rows == min(70, cus) and 64 < rows <= 1024, rows
            if kind == "wgrad":
                tiles, base = 2 * 5 * 7, 2
                assert min(-(-3 * cus // base), tiles // 8) == 8


HEAD32 = dict(N=2, H=61, W=67, C=32, mode="sat")
HEAD64 = dict(N=2, H=47, W=45, C=64, mode="sat")


@pytest.mark.parametrize("path,c", [
    pytest.param("head_ce_bwd:head32", dict(HEAD32, K=6), id="head32"),
    pytest.param("head_ce_bwd:split", dict(HEAD64, K=6), id="split")])
def test_direct_grads_head_bwd(ops, cus8, path, c):
    _path(tc.run_direct_head_bwd(ops, DEV, c), path)


def test_direct_grads_head_bn_bwd(ops, cus8):
    _path(tc.run_direct_head_bn_bwd(ops, DEV, dict(HEAD32, K=16, defer=1)), "head_ce_bn_bwd:head32")


# 0.5: every product exact in fp32 (prefill + 2 dW); 0.3: float32(float64(sum) * float64(0.3f)).
# adjacent: dw_out / db_out consecutive views of one buffer (one launch), else two allocations
@pytest.mark.parametrize("adjacent", [True, False], ids=["adjacent", "separate"])
@pytest.mark.parametrize("scale", [0.5, 0.3])
@pytest.mark.parametrize("c", [
    pytest.param(dict(HEAD32, K=6, defer=1), id="head32"),
    pytest.param(dict(HEAD64, K=6, defer=1), id="split")])
def test_head_wgrad_from_rows(ops, cus8, c, scale, adjacent):
    rows = tc.run_head_wgrad_from_rows(ops, DEV, c, scale, adjacent)
    assert rows >= 1


# rows whose sums do not fit fp32 (the slab values), through reduce_rows' wide and multi-level
# forms; the head's own shape: 6 classes x 32 channels + 6 = 198 columns
@pytest.mark.parametrize("R,adjacent", [(3, True), (300, False), (4097, True)])
def test_head_wgrad_from_rows_scales_in_fp64(ops, R, adjacent):
    tc.run_head_wgrad_synthetic(ops, DEV, R, 6, 32, 0.3, adjacent)


# ------------------------------------------------------------------ colsum_rows
# the concat data gradients of test_kernels_exact_gpu.py: dUp = the first co1 channels
COLSUM = [
    D("colsum", "conv3_fwd:res:v7:split", N=2, H=40, W=24, Cin=96, Cout=32, co1=64),
    D("colsum", "conv3_fwd:res:v1:split", N=2, H=50, W=40, Cin=160, Cout=32, co1=128),
    D("colsum", "conv3_fwd:res:v1:split", N=2, H=50, W=40, Cin=48, Cout=32, co1=16),
    D("colsum", "conv3_fwd:stream:cfg1:ks1", N=2, H=12, W=40, Cin=64, Cout=32, co1=32),
]


@pytest.mark.parametrize("kind,path,c", COLSUM)
def test_convt_bias_from_colsum_rows(ops, cus8, kind, path, c):
    dpath, wpath = tc.run_colsum(ops, DEV, c)
    _path(dpath, path)
    if DEV == "cuda":
        assert wpath.startswith("convt_wgrad:")


def test_convt_bias_from_colsum_rows_fused(ops, cus8):
    dpath, wpath = tc.run_colsum(ops, DEV, dict(N=2, H=40, W=24, Cin=96, Cout=32, co1=64), fused=True)
    _path(dpath, "conv3_fwd:res:v7:split")
    _path(wpath, "convt_bwd_fused:fused")


# ------------------------------------------------------------------ the scalars
@pytest.mark.parametrize("gs", [None, 1.0, 0.5, 0.3])
@pytest.mark.parametrize("cnt", [0, 1, 3, 4096, 12291, -2])
def test_head_grad_scale(ops, cnt, gs):
    tc.run_head_grad_scale(ops, DEV, cnt, gs)


def test_meter_add(ops):
    tc.run_meter_add(ops, DEV)


# ------------------------------------------------------------------ bindings
# the checks both registrations share (csrc/tail_checks.h); one refused call per check
def binding_calls(o, dev):
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    slab, dst = f32(4, 12), f32(12)
    rs = o.reduce_rows_scatter
    return {
        "slab-bf16": lambda: rs(slab.bfloat16(), 4, 12, dst, 2, 0, 0, False, -1),
        "slab-strided": lambda: rs(f32(12, 4).t(), 4, 12, dst, 2, 0, 0, False, -1),
        "slab-short": lambda: rs(f32(47), 4, 12, dst, 2, 0, 0, False, -1),
        "slab-short-ld": lambda: rs(f32(4 * 16 - 5), 4, 12, dst, 2, 0, 0, False, 16),
        "dst-fp64": lambda: rs(slab, 4, 12, dst.double(), 2, 0, 0, False, -1),
        "dst-strided": lambda: rs(slab, 4, 12, f32(24)[::2], 2, 0, 0, False, -1),
        "dst-longer": lambda: rs(slab, 4, 12, f32(13), 2, 0, 0, False, -1),
        "dst-shorter": lambda: rs(slab, 4, 12, f32(11), 2, 0, 0, False, -1),
        "mode0-not-ATB": lambda: rs(slab, 4, 12, dst, 0, 5, 2, False, -1),
        "mode1-not-ATB": lambda: rs(slab, 4, 12, dst, 1, 4, 5, False, -1),
        "mode0-T0": lambda: rs(slab, 4, 12, dst, 0, 0, 4, False, -1),
        "mode-3": lambda: rs(slab, 4, 12, dst, 3, 0, 0, False, -1),
        "mode-negative": lambda: rs(slab, 4, 12, dst, -1, 0, 0, False, -1),
        "ld-below-N": lambda: rs(slab, 4, 12, dst, 2, 0, 0, False, 11),
        "ld-0": lambda: rs(slab, 4, 12, dst, 2, 0, 0, False, 0),
        "dst-on-cpu": lambda: rs(slab, 4, 12, dst.cpu(), 2, 0, 0, False, -1),
        "slab-on-cpu": lambda: rs(slab.cpu(), 4, 12, dst, 2, 0, 0, False, -1),
        "R-negative": lambda: rs(slab, -1, 12, dst, 2, 0, 0, False, -1),
        # reduce_rows: above 64^3 rows its multi-level loop would reuse its scratch (refused,
        # never run)
        "reduce_rows-262145": lambda: o.reduce_rows(f32(262145), 262145, 1),
    }


BINDING_NAMES = ["slab-bf16", "slab-strided", "slab-short", "slab-short-ld", "dst-fp64", "dst-strided",
                 "dst-longer", "dst-shorter", "mode0-not-ATB", "mode1-not-ATB", "mode0-T0", "mode-3",
                 "mode-negative", "ld-below-N", "ld-0", "dst-on-cpu", "slab-on-cpu", "R-negative",
                 "reduce_rows-262145"]


CROSS_DEVICE = {"dst-on-cpu", "slab-on-cpu"}         # (one device on the CPU: nothing to refuse)


@pytest.mark.parametrize("name", BINDING_NAMES)
def test_binding_refuses(ops, name):
    if DEV == "cpu" and name in CROSS_DEVICE:
        pytest.skip("a cross-device call needs a second device")
    calls = binding_calls(ops, DEV)
    assert sorted(calls) == sorted(BINDING_NAMES)
    with pytest.raises(RuntimeError):
        calls[name]()
    if DEV == "cuda":
        torch.cuda.synchronize()


def test_binding_accepts(ops):
    """the valid neighbours of the refused calls run (the refusals are not refusing everything)"""
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    ops.reduce_rows_scatter(f32(4, 12), 4, 12, f32(12), 0, 3, 2, False, -1)
    ops.reduce_rows_scatter(f32(4 * 16 - 4), 4, 12, f32(12), 1, 2, 3, True, 16)
    assert float(ops.reduce_rows(f32(262144) + 1, 262144, 1)[0]) == 262144.0


def test_report():
    """(prints the records for docs/TESTING.md)"""
    r = tc.RECORD
    print(f"worst sum |x| per column     {r['abs_sum']:.0f} = 2^{torch.tensor(max(r['abs_sum'], 1.0)).log2():.2f}")
    print(f"worst |result| / 2^24        {r['result']:.4f}")
    by_r = {}
    for (R, N), s in r["share"].items():
        lo, hi = by_r.get(R, (1.0, 0.0))
        by_r[R] = (min(lo, s), max(hi, s))
    for R in sorted(by_r):
        print(f"fp32 accumulation wrong, R = {R:5d}: {by_r[R][0]:.2f} .. {by_r[R][1]:.2f} of the columns")
    for R, s in sorted(r["scale_share"].items()):
        print(f"scaling in fp32 wrong,   R = {R:5d}: {s:.2f} of the columns")
