"""The ``psgd_*`` operators on the CPU kernels of ``csrc/cpu_ref.cpp`` (bodies and bounds:
``powersgd_cases.py``; docs/TESTING.md, "PowerSGD codec"); ``test_powersgd_gpu.py`` is the GPU's copy."""
import pytest

import powersgd_cases as pc
from exact_cases import ops

@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_case(case):
    case[0](ops(), "cpu", *case[1:])
