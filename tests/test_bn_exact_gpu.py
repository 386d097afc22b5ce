"""Exact tests of the BatchNorm kernels: pooled routing on tied windows, every backward and apply
variant, the per-micro-batch groups, the statistics / finalize chain and the running statistics
(``bn_cases.py`` explains the method; docs/TESTING.md, "BatchNorm", lists the cases and bounds).

The norm tests of ``test_kernels_gpu.py`` hold the pooled backward to ``rel_err < 2e-2`` on
Gaussian data, where about 1 % of the windows are tied: a kernel that routes ``dP`` to the last
maximum passes them.  Here ternary inputs make 15-50 % of the windows tied, every sum exact, and
a single misrouted pixel fails.

Every case of an operator that reports one names the ``torch.ops.ddlpc.last_path()`` it is
written for and asserts it after the call (GPU only; the CPU kernels report ``cpu``): change the
SHAPE if a launcher moves a case, never the expectation.  ``test_bn_exact_cpu.py`` runs this module
on the CPU kernels (same text, DEV = "cpu"), which also proves every precondition and reference
without a GPU.
"""
import time

import pytest
import torch

import bn_cases as bc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    return bc.ops()


def C(kind, path, *shape, **c):
    cid = f"{kind}-{path}-" + "x".join(map(str, shape)) + "".join(f"-{k}{v}" for k, v in c.items())
    if shape:
        c["shape"] = shape
    c["id"] = cid
    return pytest.param(kind, path, c, id=cid)


def pooled(path, *shape, **c):
    """a pooled backward case: with dA + dP, and with dP alone"""
    keep = {k: v for k, v in c.items() if k in ("groups", "trips")}
    return [C("bwd", path, *shape, pool=1, **c), C("bwd", path, *shape, pool=1, dA=False, **keep)]


B, GB = "bn_backward:", "bn_group_backward:"
BACKWARD = [
    # ---- v2 flat (bn_bwd2_kernel<2, false>; 3-D runs it over the N * D slices)
    C("bwd", B + "v2", 2, 9, 7, 16, prefill=1),
    C("bwd", B + "v2", 2, 9, 7, 16, gscale=1),
    C("bwd", B + "v2", 3, 10, 22, 256, trips=(4, 1)),
    C("bwd", B + "v2:3d", 2, 3, 5, 7, 8),
    # ---- v2 pool, lane pair (the kw partner is lane ^ G): G = 1, 4, 32; 3-D G = 2, 32
    *pooled(B + "v2:pool", 2, 6, 10, 8, gscale=1),
    *pooled(B + "v2:pool", 2, 10, 14, 32, prefill=1),
    *pooled(B + "v2:pool", 3, 6, 10, 256, trips=(6, 1)),
    *pooled(B + "v2:pool:3d", 2, 4, 6, 10, 16, gscale=1),
    *pooled(B + "v2:pool:3d", 2, 2, 4, 6, 256),
    # ---- v2 pool, KWIN (G > 32: both kw pixels in the lane); 3-D is the UNROLL = 1 instantiation
    *pooled(B + "v2:pool:kwin", 2, 6, 10, 512, gscale=1, trips=(4, 1)),
    *pooled(B + "v2:pool:kwin", 2, 4, 6, 2048, trips=(6, 1)),
    # (its apply grid is sized for two units in flight, so the apply pass loops as well)
    *pooled(B + "v2:pool:kwin:3d", 2, 2, 4, 6, 512, gscale=1, trips=(3, 2)),
    # ---- v1 (bn_bwd_kernel): C / 8 not a power of two
    C("bwd", B + "v1", 2, 9, 7, 24, gscale=1),
    *pooled(B + "v1:pool", 2, 6, 10, 24, gscale=1),
    *pooled(B + "v1:pool", 2, 6, 10, 96, prefill=1, trips=(2, 1)),
    *pooled(B + "v1:pool:3d", 2, 2, 4, 6, 40),
    # ---- precomputed partial rows: the one-kernel finalize and the two-pass one (> 2 048 rows)
    C("bwd", B + "v2:rows", 2, 9, 7, 16, rows=3),
    C("bwd", B + "v2:rows:two_pass", 2, 9, 7, 16, rows=2049, prefill=1),
    # ---- groups (the batch = the groups' tensors one after another, [G][4][C] constants)
    *pooled(GB + "v2:pool:groups", 6, 10, 14, 32, groups=3, prefill=1),
    *pooled(GB + "v2:pool:kwin:groups", 5, 6, 10, 512, groups=5),
    *pooled(GB + "v2:pool:3d:groups", 4, 4, 6, 10, 16, groups=2),
    C("bwd", GB + "v2:groups", 6, 9, 7, 64, groups=3),
    C("bwd", GB + "v2:rows:groups", 6, 9, 7, 64, groups=3, rows=3, prefill=1),
    *pooled(GB + "v2:pool:groups", 50, 8, 8, 64, groups=50),
    # ---- bn_grad_coefs from integer rows
    C("coefs", "bn_grad_coefs:rows", 2, 9, 7, 16, rows=3),
    C("coefs", "bn_grad_coefs:two_pass", 2, 9, 7, 16, rows=2049, prefill=1),
]

A, GA = "bn_relu_apply:", "bn_group_apply:"
APPLY = [
    C("apply", A + "flat", 2, 9, 7, 16),
    C("apply", A + "flat:3d", 2, 3, 5, 7, 8),
    C("apply", A + "pool2", 2, 6, 10, 8, pool=1),
    C("apply", A + "pool2", 2, 10, 14, 32, pool=1),
    C("apply", A + "pool2", 3, 6, 10, 256, pool=1),
    C("apply", A + "pool2", 2, 10, 14, 32, pool=1, full=False),
    C("apply", A + "pool2:3d", 2, 4, 6, 10, 16, pool=1),
    C("apply", A + "pool", 2, 6, 10, 512, pool=1),
    C("apply", A + "pool", 2, 6, 10, 24, pool=1),
    C("apply", A + "pool", 2, 6, 10, 24, pool=1, full=False),
    C("apply", A + "pool:3d", 2, 2, 4, 6, 40, pool=1),
    C("apply", GA + "pool2:groups", 6, 10, 14, 32, pool=1, groups=3),
    C("apply", GA + "pool2:groups", 50, 8, 8, 64, pool=1, groups=50),
    C("apply", GA + "pool:groups", 5, 6, 10, 512, pool=1, groups=5),
    C("apply", GA + "pool2:3d:groups", 4, 4, 6, 10, 16, pool=1, groups=2),
    C("apply", GA + "flat:groups", 6, 9, 7, 64, groups=3),
]

FINALIZE = [
    C("finalize", "bn_finalize:rows", P=1, C=8, count=1),
    *[C("finalize", "bn_finalize:rows" if P <= 4096 else "bn_finalize:two_pass", P=P, C=Cn, count=cnt)
      for P, cnt in ((1, 63), (7, 441), (300, 2070), (4097, 12291)) for Cn in (8, 72)],
]

CASES = BACKWARD + APPLY + FINALIZE

# The coverage condition: every path the BatchNorm launchers can report (test_paths_covered).
PATHS = [
    "bn_relu_apply:flat", "bn_relu_apply:flat:3d", "bn_relu_apply:pool2", "bn_relu_apply:pool2:3d",
    "bn_relu_apply:pool", "bn_relu_apply:pool:3d",
    "bn_group_apply:flat:groups", "bn_group_apply:pool2:groups", "bn_group_apply:pool2:3d:groups",
    "bn_group_apply:pool:groups",
    "bn_backward:v2", "bn_backward:v2:3d", "bn_backward:v2:pool", "bn_backward:v2:pool:3d",
    "bn_backward:v2:pool:kwin", "bn_backward:v2:pool:kwin:3d",
    "bn_backward:v1", "bn_backward:v1:pool", "bn_backward:v1:pool:3d",
    "bn_backward:v2:rows", "bn_backward:v2:rows:two_pass",
    "bn_group_backward:v2:groups", "bn_group_backward:v2:rows:groups", "bn_group_backward:v2:pool:groups",
    "bn_group_backward:v2:pool:kwin:groups", "bn_group_backward:v2:pool:3d:groups",
    "bn_finalize:rows", "bn_finalize:two_pass", "bn_grad_coefs:rows", "bn_grad_coefs:two_pass",
]

RUNNERS = {"bwd": bc.run_backward, "coefs": bc.run_grad_coefs, "apply": bc.run_apply,
           "finalize": bc.run_finalize}


@pytest.mark.parametrize("kind,path,c", CASES)
def test_exact(ops, kind, path, c):
    got = RUNNERS[kind](ops, DEV, c)
    if DEV == "cuda":
        assert got == path, f"shape dispatched to {got!r}, written for {path!r}: change the shape"
    else:
        assert got == "cpu"


def test_paths_covered():
    """every listed dispatch path has a case that asserts it (and no case names an unlisted
    path, so the list stays the module's table of contents)"""
    asserted = {p.values[1] for p in CASES}
    assert sorted(set(PATHS) - asserted) == [], "paths without a case"
    assert sorted(asserted - set(PATHS)) == [], "cases whose path is not listed"
    assert len(PATHS) == len(set(PATHS))


# bn_group_finalize / bn_group_finalize_rows (they report no path: one kernel pair for every shape)
GROUP_FINALIZE = [
    dict(id="g3-63px", shape=(3, 9, 7, 8), groups=3, nb=1),            # odd: the 2-in-flight loop's tail
    dict(id="g2-2070px", shape=(4, 23, 45, 8), groups=2, nb=1),
    dict(id="g2-4158px", shape=(4, 33, 63, 8), groups=2, nb=2),        # two partial rows per group
    dict(id="g5-c256", shape=(5, 13, 11, 256), groups=5, nb=2),
    dict(id="g2-c2048", shape=(2, 5, 3, 2048), groups=2, nb=1),
]


@pytest.mark.parametrize("c", GROUP_FINALIZE, ids=lambda c: c["id"])
def test_group_finalize(ops, c):
    bc.run_group_finalize(ops, DEV, c)


RUNNING = [
    dict(id="apply-exact", Cs=[8, 24, 72], K=5, exact=True),
    dict(id="apply-gauss", Cs=[8, 24, 72], K=7, exact=False),
    dict(id="all-exact", Cs=[8, 24, 72, 16], K=5, exact=True, all=True),
    dict(id="all-gauss", Cs=[8, 24, 72, 16], K=7, exact=False, all=True),
]


@pytest.mark.parametrize("c", RUNNING, ids=lambda c: c["id"])
def test_running_apply(ops, c):
    bc.run_running(ops, DEV, c)


# ---------------------------------------------------------------------------------------------
# The kernels and their CPU twins run one text (csrc/bn_math.h): on the inputs of the cases above
# the two registrations return the same bits.  GPU only (it needs both).
AGREE = (
    [("finalize", p.values[2]) for p in FINALIZE]
    + [("group_finalize", c) for c in GROUP_FINALIZE]
    + [("running", c) for c in RUNNING if not c["exact"]]
    + [("coefs", p.values[2]) for p in BACKWARD if p.values[0] == "coefs"]
    + [("group_rows", dict(id="g3-rows3", shape=(6, 9, 7, 64), groups=3, rows=3))])
AGREE_RUNNERS = {"finalize": bc.agree_finalize, "group_finalize": bc.agree_group_finalize,
                 "running": bc.agree_running, "coefs": bc.agree_grad_coefs,
                 "group_rows": bc.agree_group_backward_rows}


@pytest.mark.parametrize("kind,c", AGREE, ids=[f"{k}-{c['id']}" for k, c in AGREE])
def test_backends_agree(ops, kind, c):
    AGREE_RUNNERS[kind](ops, c)


# ---------------------------------------------------------------------------------------------
# Above the apply pass's grid cap.  bn_bwd_apply_launch caps the grid at 8 192 workgroups; a
# trip of the flat kernel covers 8 192 x 256 lanes x 2 units in flight x 8 channels = 33.5 M
# elements, so its second trip (and the ok[1] tail behind it) runs only above that: flagship
# batches (4 x 512 x 512 x 32) do.  GPU only (the CPU kernels have no grid).
BIG = (4, 512, 520, 32)


@pytest.mark.parametrize("pool", [False, True], ids=["flat", "pool"])
def test_backward_apply_second_trip(ops, pool):
    # flat: 5 reduce trips, 2 apply trips; pooled: a lane handles both rows of the window, a trip
    # covers twice as much and the apply pass makes one trip (its reduce pass makes 3)
    assert bc.bwd_trips(BIG, pool) == ((3, 1) if pool else (5, 2))
    t0 = time.perf_counter()
    path = bc.run_backward_big(ops, DEV, BIG, pool)
    print(f"second-trip case pool={pool}: {time.perf_counter() - t0:.1f} s")
    assert path == ("bn_backward:v2:pool" if pool else "bn_backward:v2")


# ---------------------------------------------------------------------------------------------
# The argument checks both registrations share (csrc/tail_checks.h): one refused call per check.
@pytest.mark.parametrize("name", bc.BINDING_NAMES)
def test_binding_refuses(ops, name):
    if DEV == "cpu" and bc.CROSS_DEVICE in name:
        pytest.skip("a cross-device call needs a second device")
    call = bc.binding_calls(ops, DEV)[name]
    with pytest.raises(RuntimeError):
        call()
    if DEV == "cuda":
        torch.cuda.synchronize()


def test_binding_accepts(ops):
    """the valid neighbours of the refused calls run (the refusals are not refusing everything)"""
    bc.binding_accepts(ops, DEV)


def test_report():
    """(prints the records for docs/TESTING.md: worst error / bound per family, tie shares)"""
    for k in sorted(bc.WORST):
        print(f"worst error / bound  {k:40s} {bc.WORST[k]:.3f}")
    if bc.TIES:
        print("tie shares: min %.3f / %.3f, max %.3f / %.3f over %d pooled cases" % (
            min(a for a, _ in bc.TIES.values()), min(b for _, b in bc.TIES.values()),
            max(a for a, _ in bc.TIES.values()), max(b for _, b in bc.TIES.values()), len(bc.TIES)))
