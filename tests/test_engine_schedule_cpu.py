"""The schedule suite of ``test_engine_schedule_gpu.py`` run on the CPU kernels: the same text
with ``DEV = "cpu"``, where it covers every configuration of ``schedule_cases.py`` — each one's
trace against the golden file, and direct against returned gradients bit for bit.

CPU only: switches that select another kernel for the same arithmetic.  The CPU kernels share one
implementation behind those, so both settings must give identical bits; on the GPU the two kernels
sum in different orders.
"""
import os

import pytest

_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_engine_schedule_gpu.py")
_src = open(_path).read()
assert 'DEV = "cuda"' in _src and "pytestmark = pytest.mark.gpu" in _src
_src = _src.replace("pytestmark = pytest.mark.gpu", "pytestmark = []", 1).replace(
    'DEV = "cuda"', 'DEV = "cpu"', 1)
exec(compile(_src, _path, "exec"), globals())


@pytest.mark.parametrize("a,b", sc.IDENTICAL_PAIRS, ids=[f"{a}-{b}" for a, b in sc.IDENTICAL_PAIRS])
@pytest.mark.parametrize("direct", [False, True], ids=["returned", "direct"])
def test_switch_pairs_give_identical_results(a, b, direct):
    assert sc.same_results(sc.run(a, direct, DEV), sc.run(b, direct, DEV)) == []


@pytest.mark.parametrize("switch", sc.SWITCHES)
def test_every_switch_changes_the_schedule(switch):
    """No configuration is vacuous: each switch takes the step off one path onto another (with
    direct gradients; the 32-output-channel concat kernel is eligible at tile 64 only)."""
    on, off = (("tile64", "tile64_c32_bnp_off") if switch == "c32_bnp" else
               ("default", switch + "_off"))
    assert sc.run(on, True, DEV).names != sc.run(off, True, DEV).names
