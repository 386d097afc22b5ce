"""The class-weight suite of ``test_head_weighted_gpu.py`` run against the CPU kernels
(``csrc/cpu_ref.cpp``): the same text with ``DEV = "cpu"`` (the mechanism of
``test_head_exact_cpu.py``).  Both kernels of every operator are held to the same weighted fp64
reference, and every case's precondition is proven here before a GPU is touched.  Path and loop
assertions apply to the GPU kernels only (the CPU kernels report ``cpu``).
"""
import os

import pytest

_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_head_weighted_gpu.py")
_src = open(_path).read()
assert 'DEV = "cuda"' in _src and "pytestmark = pytest.mark.gpu" in _src
_src = _src.replace("pytestmark = pytest.mark.gpu", "pytestmark = []", 1).replace(
    'DEV = "cuda"', 'DEV = "cpu"', 1)
exec(compile(_src, _path, "exec"), globals())
