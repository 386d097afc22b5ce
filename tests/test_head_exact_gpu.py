"""Exact and per-element tests of the 1x1 head / cross-entropy operators (``csrc/head_ce.hip``):
the channel-split kernels for C in {8, 16, 64} and the MFMA ``head32_*`` kernels for C = 32.

``test_kernels_gpu.py`` holds these operators to whole-tensor norms at a few thousand pixels,
where no persistent loop iterates, and partly to each other.  Here every operator is compared
with an fp64 reference (``head_cases.py``): bit for bit in the saturated integer regime, under
derived per-element bounds on Gaussian data, at shapes where the persistent loops wrap — each
looping case asserts that from the row count the operator returned.  Edge cases: every pixel
ignored, whole workgroups ignored, another ignore value, one class, exact arg-max ties.

Every case names the ``last_path()`` it is written for and asserts it after the call (the CPU
kernels report ``cpu``); ``PATHS`` is the table of contents, held against the cases by
``test_paths_covered``.  A module fixture pins ``num_cus()`` to 8.

``test_head_exact_cpu.py`` runs this module on the CPU kernels (same text, DEV = "cpu").
"""
import contextlib

import pytest

import exact_cases as xc
import head_cases as hc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    return xc.ops()


@contextlib.contextmanager
def cu_reserve(o, cus):
    """run with num_cus() pinned to `cus`; reserve 0 restored after"""
    if DEV != "cuda":
        yield
        return
    try:
        phys = int(o.set_cu_reserve(0))
        o.set_cu_reserve(phys - cus)
        assert int(o.set_cu_reserve(-1)) == cus
        yield
    finally:
        o.set_cu_reserve(0)


@pytest.fixture(scope="module")
def cus8(ops):
    with cu_reserve(ops, 8):
        yield


def H(op, path, mode, loop=True, **c):
    c["mode"] = mode
    if mode == "gauss":
        c.setdefault("spread", 0.3)
    return pytest.param(op, path, loop, c, id=f"{op}-{path}-" + "x".join(
        str(c[k]) for k in ("N", "H", "W")) + "".join(
        f"-{k}{v}" for k, v in c.items() if k not in ("N", "H", "W")))


# shapes: head32 8 174 pixels = 511 wave steps with a 14-pixel tail; the apply kernel's 4-deep
# pipeline needs more than 4 x 4 x (8 workgroups x 8 CUs) steps: 16 926 pixels; channel-split
# P > 2 x rows x 256 / (C / 8) at up to 8 workgroups per CU, odd pixel counts
S32 = dict(N=2, H=61, W=67, C=32)
S32A = dict(N=2, H=91, W=93, C=32)
S64 = dict(N=2, H=47, W=45, C=64)
S16 = dict(N=2, H=91, W=95, C=16)
S8 = dict(N=2, H=129, W=129, C=8)
G3 = dict(N=9, H=20, W=44, C=32, groups=3, defer=1)        # 3 groups of 3 x 880 pixels
G5 = dict(N=10, H=20, W=44, C=32, groups=5, defer=1)       # 5 groups: 32 / 5 workgroups truncates

CASES = [
    # ---- head_logits (grid min(ceil(P / 256), 4 096): the cap's wrap is the last case)
    H("logits", "head_logits", "sat", False, **S32, K=6),
    H("logits", "head_logits:defer", "sat", False, **S64, K=11, defer=1),
    H("logits", "head_logits", "gauss", False, **S8, K=16, spread=4.0),
    H("logits", "head_logits:defer", "gauss", False, **S32, K=6, defer=1),
    H("logits", "head_logits", "sat", False, N=2, H=725, W=727, C=8, K=2),
    # ---- head_ce_fwd: the 2 048 x 256 grid-stride loop with a tail in the large cases
    H("fwd", "head_ce_fwd:split", "sat", False, **S32, K=6),
    H("fwd", "head_ce_fwd:split:defer", "sat", False, **S64, K=11, defer=1),
    H("fwd", "head_ce_fwd:split", "sat", N=2, H=515, W=511, C=8, K=2),
    H("fwd", "head_ce_fwd:split:defer", "gauss", False, **S32, K=6, defer=1),
    H("fwd", "head_ce_fwd:split", "gauss", False, **S16, K=3, spread=4.0),
    # ---- head_ce_bwd, C = 32
    H("bwd", "head_ce_bwd:head32", "sat", **S32, K=6),
    H("bwd", "head_ce_bwd:head32:defer", "sat", **S32, K=16, defer=1),
    H("bwd", "head_ce_bwd:head32:defer:stats", "sat", **S32, K=3, defer=1, store=0),
    H("bwd", "head_ce_bwd:head32", "gauss", **S32, K=6, spread=4.0),
    H("bwd", "head_ce_bwd:head32:defer", "gauss", **S32, K=6, defer=1),
    H("bwd", "head_ce_bwd:head32:defer:stats", "gauss", **S32, K=16, defer=1, store=0, spread=4.0),
    # ---- head_ce_bwd, channel-split
    H("bwd", "head_ce_bwd:split", "sat", **S64, K=6),
    H("bwd", "head_ce_bwd:split:defer", "sat", **S64, K=11, defer=1),
    H("bwd", "head_ce_bwd:split:defer:stats", "sat", **S16, K=3, defer=1, store=0),
    H("bwd", "head_ce_bwd:split", "sat", **S8, K=2),
    H("bwd", "head_ce_bwd:split:defer", "sat", **S8, K=16, defer=1),
    H("bwd", "head_ce_bwd:split", "gauss", **S16, K=3),
    H("bwd", "head_ce_bwd:split:defer", "gauss", **S64, K=6, defer=1, spread=4.0),
    H("bwd", "head_ce_bwd:split:defer:stats", "gauss", **S8, K=2, defer=1, store=0),
    # ---- head_ce_fwd_stats (unit gradient scale: K <= 6 keeps the rows below 2^24 q)
    H("fwd_stats", "head_ce_fwd_stats:head32", "sat", **S32, K=6, defer=1),
    H("fwd_stats", "head_ce_fwd_stats:head32", "sat", **S32, K=3, defer=1, seed=11),
    H("fwd_stats", "head_ce_fwd_stats:head32:groups", "sat", **G3, K=6),
    H("fwd_stats", "head_ce_fwd_stats:head32:groups", "sat", **G5, K=3),
    H("fwd_stats", "head_ce_fwd_stats:split", "sat", **S64, K=6, defer=1),
    H("fwd_stats", "head_ce_fwd_stats:split", "sat", **S16, K=3, defer=1),
    H("fwd_stats", "head_ce_fwd_stats:split", "sat", **S8, K=2, defer=1),
    H("fwd_stats", "head_ce_fwd_stats:head32", "gauss", **S32, K=6, defer=1),
    H("fwd_stats", "head_ce_fwd_stats:head32", "gauss", **S32, K=16, defer=1, spread=4.0),
    H("fwd_stats", "head_ce_fwd_stats:head32:groups", "gauss", **G5, K=6),
    H("fwd_stats", "head_ce_fwd_stats:split", "gauss", **S64, K=6, defer=1, spread=4.0),
    # ---- head_ce_bn_bwd
    H("bn_bwd", "head_ce_bn_bwd:head32", "sat", **S32A, K=6, defer=1),
    H("bn_bwd", "head_ce_bn_bwd:head32", "sat", False, **S32, K=16, defer=1),
    H("bn_bwd", "head_ce_bn_bwd:head32:groups", "sat", **G3, K=6),
    H("bn_bwd", "head_ce_bn_bwd:head32:groups", "sat", **G5, K=3),
    H("bn_bwd", "head_ce_bn_bwd:split", "sat", False, **S64, K=11, defer=1),
    H("bn_bwd", "head_ce_bn_bwd:split", "sat", False, **S8, K=2, defer=1),
    # the 4 096-workgroup cap of the channel-split apply kernel wraps above 4 096 x 4 x 32 pixels
    H("bn_bwd", "head_ce_bn_bwd:split", "sat", N=2, H=513, W=513, C=64, K=2, defer=1),
    H("bn_bwd", "head_ce_bn_bwd:head32", "gauss", **S32A, K=6, defer=1, spread=4.0),
    H("bn_bwd", "head_ce_bn_bwd:head32:groups", "gauss", **G3, K=6),
    H("bn_bwd", "head_ce_bn_bwd:split", "gauss", False, **S16, K=3, defer=1),
]

# Edge cases, each on head32 and on one channel-split shape
_EDGE_OPS = [("fwd", "head_ce_fwd:split:defer"), ("bwd", "head_ce_bwd:{v}:defer"),
             ("fwd_stats", "head_ce_fwd_stats:{v}"), ("bn_bwd", "head_ce_bn_bwd:{v}")]
_EDGES = [
    dict(mode="sat", ignored="all", K=6),                    # count = 0, gs = gscale / 1
    dict(mode="sat", lead=1024, K=6),                        # whole workgroups of ignored pixels
    dict(mode="sat", ignore_index=255, K=6),                 # labels that contain 255
    dict(mode="sat", K=1),                                   # loss 0, gradients 0, hits = count
    dict(mode="tie", tie=(1, 4), K=6, ignored="some"),       # first maximum
]
EDGE_CASES = [H(op, path.format(v=v), e["mode"], False, **s, defer=1,
                **{k: x for k, x in e.items() if k != "mode"})
              for e in _EDGES for v, s in (("head32", S32), ("split", S64)) for op, path in _EDGE_OPS]

PATHS = [
    "head_logits", "head_logits:defer",
    "head_ce_fwd:split", "head_ce_fwd:split:defer",
    "head_ce_bwd:head32", "head_ce_bwd:head32:defer", "head_ce_bwd:head32:defer:stats",
    "head_ce_bwd:split", "head_ce_bwd:split:defer", "head_ce_bwd:split:defer:stats",
    "head_ce_fwd_stats:head32", "head_ce_fwd_stats:head32:groups", "head_ce_fwd_stats:split",
    "head_ce_bn_bwd:head32", "head_ce_bn_bwd:head32:groups", "head_ce_bn_bwd:split",
]


def _run(ops, op, path, loop, c):
    got, info = hc.RUNNERS[op](ops, DEV, c)
    if DEV != "cuda":
        assert got == "cpu"
        return
    assert got == path, f"shape dispatched to {got!r}, written for {path!r}: change the shape"
    if loop:
        have, need = hc.loops(op, c, info)
        assert have > need, f"the case does not loop: {have} <= {need} (rows / grid: {info})"


@pytest.mark.parametrize("op,path,loop,c", CASES)
def test_head(ops, cus8, op, path, loop, c):
    _run(ops, op, path, loop, c)


@pytest.mark.parametrize("op,path,loop,c", EDGE_CASES)
def test_head_edge(ops, cus8, op, path, loop, c):
    _run(ops, op, path, loop, c)


def test_all_ignored_is_zero(ops, cus8):
    """every pixel ignored: out3 = (0, 0, 0), every gradient, row and partial exactly 0"""
    for s in (S32, S64):
        c = dict(s, K=6, defer=1, mode="sat", ignored="all")
        cs = hc.make(c)
        y, Wh, bh, lab, s4 = (t.to(DEV) for t in (cs.y, cs.Wh, cs.bh, cs.lab, cs.s4))
        out3, wrows, brows = ops.head_ce_fwd_stats(y, Wh, bh, lab, -100, s4, 0)
        assert out3.tolist() == [0.0, 0.0, 0.0]
        assert ops.head_ce_fwd(y, Wh, bh, lab, -100, s4).tolist() == [0.0, 0.0, 0.0]
        outs = list(ops.head_ce_bwd(y, Wh, bh, lab, out3, None, -100, None, None, s4))
        outs += list(ops.head_ce_bn_bwd(y, Wh, bh, lab, out3, None, -100, s4, outs[3], cs.gamma.to(DEV)))
        for t in [wrows, brows] + outs:
            assert t.numel() and int((t != 0).sum()) == 0


def test_paths_covered():
    """every head path has a saturated and a Gaussian case that asserts it, and no case names
    an unlisted path"""
    by_mode = {}
    for p in CASES + EDGE_CASES:
        by_mode.setdefault(p.values[3]["mode"], set()).add(p.values[1])
    for mode in ("sat", "gauss"):
        assert sorted(set(PATHS) - by_mode[mode]) == [], f"paths without a {mode} case"
    asserted = set().union(*by_mode.values())
    assert sorted(asserted - set(PATHS)) == [], "cases whose path is not listed"
    assert len(PATHS) == len(set(PATHS))
