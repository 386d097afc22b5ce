"""The scheduled optimizer step ``adam_step_sched`` on the gfx950 kernels of ``csrc/optim.hip``:
gradient norm and clip coefficient (exact and general), the reduction to ``adam_step_dev``, the
clipped / decoupled update per element, the learning-rate schedule and the binding's checks
(``sched_cases.py`` holds the bodies and the method; docs/TESTING.md, "Scheduled optimizer step",
lists the cases and derives the bounds).

``test_sched_cpu.py`` runs this module on the CPU kernels (same text, DEV = "cpu").
"""
import pytest
import torch

import sched_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    return sc.ops()


# ------------------------------------------------------------------ norm
# SQ_BIG: the norm kernel's grid caps at 1 024 workgroups of 256 threads, a float4 each (SQ_TRIP =
# 1 048 576 elements per trip): two full trips, a partial third and the scalar tail
@pytest.mark.parametrize("n", sc.NORM_SIZES)
def test_norm_exact(ops, n):
    sc.run_norm_exact(ops, DEV, n)


def test_norm_exact_view(ops):
    """a view 4 099 floats into a larger buffer (16-byte misaligned for the float4 loop)"""
    sc.run_norm_exact(ops, DEV, 10_007, offset=4099)


@pytest.mark.parametrize("n", sc.NORM_SIZES)
def test_norm_general(ops, n):
    sc.run_norm_general(ops, DEV, n)


def test_norm_general_view(ops):
    sc.run_norm_general(ops, DEV, 10_007, offset=4099)


# ------------------------------------------------------------------ update
@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["wd0", "wd0.01"])
@pytest.mark.parametrize("n", [3, 1027, 10_007])
def test_reduces_to_adam_step_dev(ops, n, wd):
    sc.run_reduces(ops, DEV, n, wd)


def test_reference_is_adam_ref():
    sc.check_sched_ref()


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["wd0", "wd0.01"])
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 10_007])
def test_update(ops, n, wd, clip, decoupled):
    sc.run_update(ops, DEV, n, wd, clip, decoupled)


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_update_view(ops, decoupled):
    sc.run_update(ops, DEV, 10_007, 0.01, True, decoupled, offset=4099)


# ------------------------------------------------------------------ schedule
@pytest.mark.parametrize("kind,power", [("constant", 0.9), ("poly", 1.0), ("poly", 0.9), ("cosine", 0.9)],
                         ids=["constant", "poly1", "poly0.9", "cosine"])
def test_schedule(ops, kind, power):
    sc.run_schedule(ops, DEV, kind, power)


# ------------------------------------------------------------------ bindings
def test_empty_call(ops):
    sc.run_empty(ops, DEV)


# GPU only: the checks of the GPU binding (csrc/bindings.cpp)
@pytest.mark.parametrize("name", sc.BINDING_NAMES)
def test_binding_refuses(ops, name):
    with pytest.raises(RuntimeError):
        sc.binding_calls(ops, DEV)[name]()
    torch.cuda.synchronize()


def test_report():
    """(prints the records for docs/TESTING.md: worst error / bound per family)"""
    for k in sorted(sc.record.__globals__["WORST"]):
        if k.startswith("adam_step_sched"):
            print(f"worst error / bound  {k:46s} {sc.record.__globals__['WORST'][k]:.3f}")
