"""The ``psgd_*`` operators on the gfx950 kernels of ``csrc/powersgd.hip`` (bodies and bounds:
``powersgd_cases.py``; docs/TESTING.md, "PowerSGD codec"); ``test_powersgd_cpu.py`` is the CPU's copy."""
import pytest

import powersgd_cases as pc
from exact_cases import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_case(case):
    case[0](ops(), DEV, *case[1:])


def _exchange(dev, n, m, r, upto=5):
    return pc.Exchange(ops(), dev, n, m, r, pc.gauss(1, 1e-2), pc.gauss(2, 1e-3), pc.gauss(3)).run(upto)


@pytest.mark.parametrize("n,m,r", [(33, 257, 4), (17, 27, 4), (33, 32, 16)])
def test_residual_and_decode_match_the_cpu_kernels_bitwise(n, m, r):    # (the shared fma chain)
    o, x, y = ops(), _exchange("cuda", n, m, r, upto=2), _exchange("cpu", n, m, r, upto=2)
    for t in (x, y):                      # A = e + g is in e; P-hat and a Q from the GPU
        t.wire_p.copy_(x.wire_p)
        t.wire_q.copy_(pc.gauss(4)(t.plan.wire_q))
        o.psgd_residual(t.e, t.wire_p, t.wire_q, t.lo, r)
        o.psgd_decode(t.g, t.wire_p, t.wire_q, t.lo, t.ra, r)
    pc.assert_bits(x.e, y.e, "residual")
    pc.assert_bits(x.g, y.g, "decode")


def test_same_bits_twice_and_on_8_cus():
    o, runs = ops(), [_exchange(DEV, 33, 257, 4) for _ in range(2)]
    try:
        assert int(o.set_cu_reserve(int(o.set_cu_reserve(0)) - 8)) == 8
        runs.append(_exchange(DEV, 33, 257, 4))
    finally:
        o.set_cu_reserve(0)
    for x in runs[1:]:
        for name in ("g", "e", "wire_p", "wire_q", "q_loc"):
            pc.assert_bits(getattr(x, name), getattr(runs[0], name), name)
