"""The engine's schedule, pinned: which ``torch.ops.ddlpc`` operators one training step calls,
with which tensors, in which order, inside which ``wgrad_stream`` segment, and when each
parameter's gradient is reported ready (``schedule_cases.py`` has the tracer and the
configurations; docs/TESTING.md, "Engine schedule", says what a trace holds and when the golden
file may be regenerated).

The engine is one code path over two kernel sets, so a trace is device-independent: the GPU runs
three configurations (the 32-output-channel concat weight gradient at tile 64, the fused BatchNorm
groups, 3-D), each with returned and with direct gradients, against the same golden entries that
``test_engine_schedule_cpu.py`` (this text with ``DEV = "cpu"``) checks for every configuration.
"""
import pytest
import torch

import schedule_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"

NAMES = sc.GPU_CASES if DEV == "cuda" else [c["name"] for c in sc.CASES]


@pytest.fixture(scope="module")
def golden():
    return sc.golden()


@pytest.mark.parametrize("name,direct", [pytest.param(n, d, id=sc.key_id(n, d))
                                         for n, d in sc.keys(NAMES)])
def test_trace_equals_golden(golden, name, direct):
    """Event names first (a readable difference), then the count and the hash of the full trace
    (arguments, tensor labels, results)."""
    r = sc.run(name, direct, DEV)
    g = golden[sc.key_id(name, direct)]
    assert r.names == g["events"]
    assert r.count == g["count"]
    assert r.sha256 == g["sha256"], "operator arguments or data flow changed: diff two --dump runs"


@pytest.mark.parametrize("name", [n for n in NAMES if n in sc.TRAIN])
def test_direct_gradients_equal_returned(name):
    """Kernels accumulating into zeroed ``.grad`` buffers leave the bits autograd is handed
    otherwise: loss, hit count, every parameter gradient and every buffer."""
    assert sc.same_results(sc.run(name, False, DEV), sc.run(name, True, DEV)) == []
