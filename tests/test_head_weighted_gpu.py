"""Class-weighted cross-entropy through the head operators (``class_weight=``;
``csrc/head_ce.hip``): every path with a loss or a gradient against the weighted fp64 reference
of ``head_weight_cases.py`` — bit for bit in the saturated regime (weights from {1/2, 1, 2}, a
power-of-two weight sum), under per-element bounds on Gaussian data (arbitrary weights, one of
them 0) — plus the identities that pin the unweighted path (None = all ones = argument omitted;
all twos: the same loss and gradients, a doubled weight sum) and the edge runs (labels equal to
ignore_index = 255, every pixel ignored, every valid label of weight 0).

Every case asserts the ``last_path()`` it is written for; ``num_cus()`` is pinned to 8 as in
``test_head_exact_gpu.py``.  ``test_head_weighted_cpu.py`` runs this module on the CPU kernels
(same text, DEV = "cpu").
"""
import contextlib

import pytest
import torch

import exact_cases as xc
import head_cases as hc
import head_weight_cases as wc
from head_weight_cases import G3, G5, S8, S16, S32, S32A, S64

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


def H(op, path, loop=True, **c):
    return (op, path, loop, c)


# one case per path with a loss or a gradient, at the shapes the unweighted suite derived for
# that path (K chosen so that both regimes' preconditions hold).  Each entry runs in both regimes.
PATH_CASES = [
    H("fwd", "head_ce_fwd:split", False, **S32, K=6),
    H("fwd", "head_ce_fwd:split:defer", False, **S64, K=6, defer=1),
    H("bwd", "head_ce_bwd:head32", **S32, K=6),
    H("bwd", "head_ce_bwd:head32:defer", **S32, K=6, defer=1),
    H("bwd", "head_ce_bwd:head32:defer:stats", **S32, K=3, defer=1, store=0),
    H("bwd", "head_ce_bwd:split", **S64, K=6),
    H("bwd", "head_ce_bwd:split:defer", **S64, K=11, defer=1),
    H("bwd", "head_ce_bwd:split:defer:stats", **S16, K=3, defer=1, store=0),
    H("fwd_stats", "head_ce_fwd_stats:head32", **S32, K=6, defer=1),
    H("fwd_stats", "head_ce_fwd_stats:head32:groups", **G3, K=6),
    H("fwd_stats", "head_ce_fwd_stats:split", **S64, K=6, defer=1),
    H("bn_bwd", "head_ce_bn_bwd:head32", **S32A, K=6, defer=1),
    H("bn_bwd", "head_ce_bn_bwd:head32:groups", **G5, K=3),
    H("bn_bwd", "head_ce_bn_bwd:split", False, **S8, K=2, defer=1),
]

# the paths of test_head_exact_gpu.py that have a loss or a gradient (head_logits has neither)
PATHS = [
    "head_ce_fwd:split", "head_ce_fwd:split:defer",
    "head_ce_bwd:head32", "head_ce_bwd:head32:defer", "head_ce_bwd:head32:defer:stats",
    "head_ce_bwd:split", "head_ce_bwd:split:defer", "head_ce_bwd:split:defer:stats",
    "head_ce_fwd_stats:head32", "head_ce_fwd_stats:head32:groups", "head_ce_fwd_stats:split",
    "head_ce_bn_bwd:head32", "head_ce_bn_bwd:head32:groups", "head_ce_bn_bwd:split",
]


def _id(p):
    op, path, loop, c = p
    return f"{path}-" + "x".join(str(c[k]) for k in ("N", "H", "W")) + f"-K{c['K']}"


def _run(ops, op, path, loop, c, w):
    got, info = wc.RUNNERS[op](ops, DEV, c, w)
    if DEV != "cuda":
        assert got == "cpu"
        return
    assert got == path, f"shape dispatched to {got!r}, written for {path!r}: change the shape"
    if loop:
        have, need = hc.loops(op, c, info)
        assert have > need, f"the case does not loop: {have} <= {need} (rows / grid: {info})"


@pytest.mark.parametrize("p", PATH_CASES, ids=_id)
def test_weighted_exact(ops, cus8, p):
    """saturated regime, weights from {1/2, 1, 2}: bit-equal to the fp64 reference"""
    op, path, loop, c = p
    c = dict(c, mode="sat")
    _run(ops, op, path, loop, c, wc.sat_weights(c["K"], c.get("seed", 7)))


@pytest.mark.parametrize("p", PATH_CASES, ids=_id)
def test_weighted_gauss(ops, cus8, p):
    """Gaussian regime, arbitrary weights (one exactly 0): per-element bounds"""
    op, path, loop, c = p
    c = dict(c, mode="gauss")
    c.setdefault("spread", 0.3)
    _run(ops, op, path, loop, c, wc.gauss_weights(c["K"]))


def test_paths_covered():
    assert sorted(p[1] for p in PATH_CASES) == sorted(PATHS) and len(PATHS) == 14


# ------------------------------------------------------------------ identities
ID_SHAPES = [("head32", dict(S32, K=6, defer=1, mode="gauss", spread=0.3)),
             ("split", dict(S64, K=6, defer=1, mode="gauss", spread=0.3))]


@pytest.fixture(scope="module")
def base_outputs(ops, cus8):
    """the unweighted outputs of every operator (class_weight=None), computed once per shape"""
    return {v: wc.all_ops(ops, DEV, hc.make(c), None, "kw") for v, c in ID_SHAPES}


@pytest.mark.parametrize("v,c", ID_SHAPES, ids=[v for v, _ in ID_SHAPES])
def test_none_ones_omitted_identical(ops, cus8, base_outputs, v, c):
    cs = hc.make(c)
    base = base_outputs[v]
    ones = wc.all_ops(ops, DEV, cs, torch.ones(cs.K, device=DEV), "kw")
    omitted = wc.all_ops(ops, DEV, cs, None, "kw", omit=True)
    assert float(base["fwd.out3"][2]) == float(hc.reference(c, 1.0).count)
    for name, t in base.items():
        assert torch.equal(t, ones[name]), f"{name}: all-ones weights differ from class_weight=None"
        assert torch.equal(t, omitted[name]), f"{name}: omitted argument differs from class_weight=None"


@pytest.mark.parametrize("v,c", ID_SHAPES, ids=[v for v, _ in ID_SHAPES])
def test_all_twos(ops, cus8, base_outputs, v, c):
    """weights of 2 everywhere: the same loss bits, a doubled weight sum, bit-identical gradients
    (the unit-scale rows of the fused forward double; their scale halves)"""
    cs = hc.make(c)
    base = base_outputs[v]
    twos = wc.all_ops(ops, DEV, cs, torch.full((cs.K,), 2.0, device=DEV), "kw")
    for name in ("fwd.out3", "fwd_stats.out3"):
        b, t = base[name], twos[name]
        assert torch.equal(b[0], t[0]) and torch.equal(b[1], t[1]), f"{name}: loss / hits changed"
        assert float(t[2]) == 2.0 * float(b[2]), f"{name}: weight sum {float(t[2])} != 2 x {float(b[2])}"
    for name in ("rows.w", "rows.bn"):
        assert torch.equal(twos[name], 2.0 * base[name]), f"{name}: unit-scale rows not doubled"
    for name in wc.GRADS:
        assert torch.equal(base[name], twos[name]), f"{name}: gradients differ under all-twos weights"


def _finite_outputs(out):
    for name, t in out.items():
        assert bool(torch.isfinite(t.float()).all()), f"{name}: non-finite values"


@pytest.mark.parametrize("v,c", ID_SHAPES, ids=[v for v, _ in ID_SHAPES])
def test_edges(ops, cus8, v, c):
    """labels equal to ignore_index = 255 (never an index into the weight table), every pixel
    ignored, every valid label of weight 0: no fault, no NaN, and the zero-weight-sum rule"""
    w = wc.gauss_weights(6).to(DEV)
    # ---- ignore_index = 255 among the labels: equal to the same pixels ignored as -100
    c255 = dict(c, ignore_index=255)
    cs255 = hc.make(c255)
    assert int((cs255.lab == 255).sum()) > 0
    out255 = wc.all_ops(ops, DEV, cs255, w, "kw")
    _finite_outputs(out255)
    csm = wc.relabel(cs255, torch.where(cs255.lab == 255, torch.full_like(cs255.lab, -100), cs255.lab))
    csm.ign = -100
    outm = wc.all_ops(ops, DEV, csm, w, "kw")
    for name, t in out255.items():
        assert torch.equal(t, outm[name]), f"{name}: ignore_index 255 differs from -100 on the same pixels"
    # ---- every pixel ignored
    csa = hc.make(dict(c, ignored="all"))
    outa = wc.all_ops(ops, DEV, csa, w, "kw")
    for name, t in outa.items():
        assert t.numel() and int((t != 0).sum()) == 0, f"{name}: not zero with every pixel ignored"
    # ---- every valid label of weight 0: loss 0, weight sum 0, gradients 0; hits unweighted
    cs = hc.make(c)
    present = torch.unique(cs.lab[cs.lab != cs.ign])
    w0 = torch.ones(cs.K)
    w0[present] = 0.0
    if bool((w0 == 0).all()):          # (every class occurs: weights that are all zero)
        w0 = torch.zeros(cs.K)
    out0 = wc.all_ops(ops, DEV, cs, w0.to(DEV), "kw")
    r = hc.reference(c, 1.0)
    for name in ("fwd.out3", "fwd_stats.out3"):
        o3 = out0[name].tolist()
        assert o3[0] == 0.0 and o3[2] == 0.0, f"{name}: {o3}"
        assert abs(o3[1] - r.hits) <= 0.001 * r.count + 1, f"{name}: hits {o3[1]} vs {r.hits}"
    for name in wc.GRADS + ["rows.w", "rows.bn"]:
        assert int((out0[name] != 0).sum()) == 0, f"{name}: not zero under zero weights"


def test_zz_report_ratios():
    """(not an assertion: the worst error / bound per family, for docs/TESTING.md)"""
    for k in sorted(hc.RATIO):
        if k.startswith("w."):
            print(f"RATIO {DEV} {k} {hc.RATIO[k]:.3g}")
    for k in sorted(xc.WORST, key=str):
        if str(k[0]).startswith("w."):
            print(f"WORST {DEV} {k} {xc.WORST[k]:.6g}")
