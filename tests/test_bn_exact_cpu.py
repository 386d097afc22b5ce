"""The BatchNorm suite of ``test_bn_exact_gpu.py`` run against the CPU kernels.

The same text with ``DEV = "cpu"`` (as ``test_kernels_exact_cpu.py`` mirrors its GPU module): both
kernels of every operator are held to the exact specification, and every case's preconditions
(multiples of the quantum, magnitude caps, tie shares) and fp64 reference are proven here before
a GPU is touched.  Path assertions apply to the GPU kernels only (the CPU kernels report ``cpu``).
"""
import os

import pytest

_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_bn_exact_gpu.py")
_src = open(_path).read()
assert 'DEV = "cuda"' in _src and "pytestmark = pytest.mark.gpu" in _src
_src = _src.replace("pytestmark = pytest.mark.gpu", "pytestmark = []", 1).replace(
    'DEV = "cuda"', 'DEV = "cpu"', 1)
exec(compile(_src, _path, "exec"), globals())

# the 34 M-element case is about the GPU apply pass's grid cap (the CPU kernels have no grid);
# test_backends_agree compares the two registrations, so it needs both
_GPU_ONLY = {"test_backward_apply_second_trip", "test_backends_agree"}
for _name in _GPU_ONLY:
    del globals()[_name]
