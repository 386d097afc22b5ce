"""The gradient-tail suite of ``test_tail_exact_gpu.py`` run against the CPU kernels.

The same text with ``DEV = "cpu"`` (as ``test_update_exact_cpu.py`` mirrors its GPU module): both
kernels of every operator are held to the same references, bit for bit, and every case's
preconditions (exactness in fp32 / fp64, the share of columns an fp32 accumulation gets wrong,
non-zero statistics halves) and references are proven here before a GPU is touched.
"""
import os

import pytest

_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_tail_exact_gpu.py")
_src = open(_path).read()
assert 'DEV = "cuda"' in _src and "pytestmark = pytest.mark.gpu" in _src
_src = _src.replace("pytestmark = pytest.mark.gpu", "pytestmark = []", 1).replace(
    'DEV = "cuda"', 'DEV = "cpu"', 1)
exec(compile(_src, _path, "exec"), globals())
