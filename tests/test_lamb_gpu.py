"""``lamb_step`` on the gfx950 kernels of ``csrc/lamb.hip`` (bodies and bounds: ``lamb_cases.py``;
docs/TESTING.md, "LAMB step").  ``test_lamb_cpu.py`` runs this text on the CPU kernels."""
import pytest

import lamb_cases as lc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("exclude_1d", [True, False], ids=["exclude1d", "all"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["wd0", "wd0.01"])
def test_stages(wd, clip, exclude_1d):
    lc.run_stages(lc.ops(), DEV, wd, clip, exclude_1d)


def test_same_bits_twice_and_captured():
    lc.run_capture()


@pytest.mark.parametrize("name", [n for n in lc.REFUSALS if DEV == "cuda" or "on the host" not in n])
def test_refuses(name):
    with pytest.raises(RuntimeError):
        lc.run_refusal(lc.ops(), DEV, name)
