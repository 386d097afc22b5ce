"""``test_head_eval_gpu.py`` on the CPU kernels (``DEV = "cpu"``, as ``test_head_dice_cpu.py``)."""
import os

import pytest

_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_head_eval_gpu.py")
_src = open(_path).read()
assert 'DEV = "cuda"' in _src and "pytestmark = pytest.mark.gpu" in _src
_src = _src.replace("pytestmark = pytest.mark.gpu", "pytestmark = []", 1).replace(
    'DEV = "cuda"', 'DEV = "cpu"', 1)
exec(compile(_src, _path, "exec"), globals())
