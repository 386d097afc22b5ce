"""The scheduled-step suite of ``test_sched_gpu.py`` run against the CPU kernels (the same text
with ``DEV = "cpu"``, as ``test_update_exact_cpu.py`` mirrors its GPU module): both kernels of the
operator are held to the same references and bounds, and every case's preconditions are proven
here before a GPU is touched.
"""
import os

import pytest

_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_sched_gpu.py")
_src = open(_path).read()
assert 'DEV = "cuda"' in _src and "pytestmark = pytest.mark.gpu" in _src
_src = _src.replace("pytestmark = pytest.mark.gpu", "pytestmark = []", 1).replace(
    'DEV = "cuda"', 'DEV = "cpu"', 1)
exec(compile(_src, _path, "exec"), globals())

# the refusals are the TORCH_CHECKs of the GPU binding
del globals()["test_binding_refuses"]
