"""Cases for the five ``psgd_*`` operators (``csrc/powersgd.hip``, CPU twins in ``csrc/cpu_ref.cpp``,
shared text in ``csrc/powersgd_math.h``), run on both kernel sets by ``test_powersgd_gpu.py`` and
``test_powersgd_cpu.py``; ``parallel/codec.py`` (``powersgd_*``) is the contract and the oracle.

Integer cases: operands are integers with |x| <= 4 and w = 1/2, so every sum is exact in fp32 in any
order and outputs must equal an int64 matmul bit for bit.  Gaussian cases: a kernel may miss the fp64
contract by ``8 ||fp32 contract - fp64||_F + ulp32(max |fp64|)`` on the same inputs (8 x: another, equally
long fp32 summation order; nothing tighter can be derived for an MFMA's internal order).
"""
import pytest
import torch

from update_cases import SENT, _gen, assert_bits, ulp32

NS, MS, RS = (6, 16, 17, 33), (27, 32, 257), (1, 4, 16)     # m: unaligned rows, one K-chunk, a chunk + 1
INT_CASES = [(n, m, r, False) for r in RS for n in NS for m in MS if (n + m) * r < n * m] + [(6, 27, 16, True)]
ORTH_ROWS = (0, 100, 300, 519)        # the 4 rows of block 0 (block j: + j) — every wave, 3 rows a thread


def bucket(n, m, r, hand=False):
    """-> (plan, floats) of one bucket at offset 64 of its flat buffer: raw 5 | n x m | raw 70 | m x n |
    n x 1 x m with the layout's gaps; ``hand``: a table the plan's rule would not admit, unaligned."""
    from ddlpc.parallel import codec as C
    if hand:
        low = torch.tensor([[3, n, m, 11, 0]], dtype=torch.int32)
        raw = torch.tensor([[3 + n * m + 2, 10, 0]], dtype=torch.int32)
        return C.PowerSGDPlan(r, low, raw, 11 + n * r, m * r, n * m + 10), 3 + n * m + 2 + 10 + 5
    from ddlpc.parallel.flat import FlatParams
    flat = FlatParams([torch.nn.Parameter(torch.zeros(s)) for s in ((n, 1, m), (m, n), (70,), (n, m), (5,), (7,))])
    start = flat.span(flat.order[1])[0]
    plan = C.powersgd_plan(flat, flat.order[1:], start, r)
    assert start == 64 and plan.low.shape[0] == 3 and plan.raw.shape[0] == 2
    return plan, flat.numel - start


def place(x, dev, shift=0):       # a copy of x on dev, ``shift`` floats past an allocation's 16-byte boundary
    buf = torch.empty(x.numel() + shift, dtype=x.dtype, device=dev)
    buf[shift:].copy_(x)
    return buf[shift:]


def ints(n, seed):
    return torch.randint(-4, 5, (n,), generator=_gen(seed)).float()


def run_int(o, dev, n, m, r, hand, shift):
    plan, size = bucket(n, m, r, hand)
    lo, ra, rows, raws = plan.low.to(dev), plan.raw.to(dev), plan.low.tolist(), plan.raw.tolist()
    inlow, inraw, sent = torch.zeros(size, dtype=torch.bool), torch.zeros(size, dtype=torch.bool), torch.tensor(SENT)
    for off, nn, mm, _, _ in rows:
        inlow[off:off + nn * mm] = True
    for off, length, _ in raws:
        inraw[off:off + length] = True
    g0 = torch.where(inlow | inraw, ints(size, 1), sent)
    e0 = torch.where(inlow, ints(size, 2), sent)
    q0, ph, qi = ints(plan.wire_q, 3), ints(plan.wire_p, 4), ints(plan.wire_q, 5)
    g, e, wire_p = place(g0, dev, shift), place(e0, dev, shift), torch.full((plan.wire_p,), SENT, device=dev)

    def mat(x, at, a, b):
        return x[at:at + a * b].view(a, b).long()

    o.psgd_project(g, e, q0.to(dev), wire_p, lo, ra, r, 0.5)
    A, want = torch.where(inlow, e0 + g0, e0), torch.full((plan.wire_p,), SENT)
    for off, nn, mm, po, qo in rows:
        want[po:po + nn * r] = 0.5 * (mat(A, off, nn, mm) @ mat(q0, qo, mm, r)).float().reshape(-1)
    for off, length, wo in raws:
        want[wo:wo + length] = 0.5 * g0[off:off + length]
    assert_bits(e, A, "project: e <- e + g, nothing else written")
    assert_bits(wire_p, want, "project: wire_p")
    assert_bits(g, g0, "project: g was written")

    wire_p.copy_(ph)                      # a P-hat supplied directly
    q_loc, wire_q = (torch.full((plan.wire_q,), SENT, device=dev) for _ in range(2))
    o.psgd_backproject(e, wire_p, q_loc, wire_q, lo, r, 0.5)
    want = torch.empty(plan.wire_q)
    for off, nn, mm, po, qo in rows:
        want[qo:qo + mm * r] = (mat(A, off, nn, mm).t() @ mat(ph, po, nn, r)).float().reshape(-1)
    assert_bits(q_loc, want, "backproject: q_loc")
    assert_bits(wire_q, 0.5 * want, "backproject: wire_q")

    o.psgd_residual(e, wire_p, qi.to(dev), lo, r)
    o.psgd_decode(g, wire_p, qi.to(dev), lo, ra, r)
    we, wg = A.clone(), g0.clone()
    for off, nn, mm, po, qo in rows:
        pq = (mat(ph, po, nn, r) @ mat(qi, qo, mm, r).t()).float().reshape(-1)
        we[off:off + nn * mm] -= pq
        wg[off:off + nn * mm] = pq
    for off, length, wo in raws:
        wg[off:off + length] = ph[wo:wo + length]
    assert_bits(e, we, "residual")
    assert_bits(g, wg, "decode")


def run_orth_exact(o, dev, r):
    """Column j holds a_j = +-2^k on the 4-row blocks 0 .. j (block b = rows ORTH_ROWS + b): every dot and norm
    is exact, q_j = sign(a_j) / 2 on block j, 0 elsewhere.  r >= 4: column 2 is zero, stays zero, is not seen."""
    n, rows = 540, torch.tensor(ORTH_ROWS)
    p, want, blk = torch.zeros(n, r), torch.zeros(n, r), 0
    for j in range(r):
        if r >= 4 and j == 2:
            continue
        a = (-1.0) ** j * 2.0 ** (j % 5 - 2)
        for b in range(blk + 1):
            p[rows + b, j] = a
        want[rows + blk, j] = 0.5 if a > 0 else -0.5
        blk += 1
    low = torch.tensor([[0, n, 1000, 5, 0]], dtype=torch.int32).to(dev)
    wire_p = torch.cat([torch.full((5,), SENT), p.reshape(-1), torch.full((3,), SENT)]).to(dev)
    o.psgd_orthonormalize(wire_p, low, r)
    assert_bits(wire_p, torch.cat([torch.full((5,), SENT), want.reshape(-1), torch.full((3,), SENT)]), "P-hat")


class Exchange:     # one bucket (the plan's n x m tensor and its neighbours) through the five operators, world 1
    def __init__(self, o, dev, n, m, r, g, e, q):
        self.o, self.r = o, r
        self.plan, size = bucket(n, m, r)
        self.lo, self.ra = self.plan.low.to(dev), self.plan.raw.to(dev)
        self.g, self.e, self.q = place(g(size), dev), place(e(size), dev), place(q(self.plan.wire_q), dev)
        self.wire_p, self.wire_q = torch.zeros(self.plan.wire_p, device=dev), torch.zeros(self.plan.wire_q, device=dev)
        self.q_loc = torch.zeros_like(self.wire_q)

    def run(self, upto=5):
        o, r = self.o, self.r
        o.psgd_project(self.g, self.e, self.q, self.wire_p, self.lo, self.ra, r, 1.0)
        o.psgd_orthonormalize(self.wire_p, self.lo, r)
        if upto > 2:
            o.psgd_backproject(self.e, self.wire_p, self.q_loc, self.wire_q, self.lo, r, 1.0)
            o.psgd_residual(self.e, self.wire_p, self.q_loc, self.lo, r)
            o.psgd_decode(self.g, self.wire_p, self.wire_q, self.lo, self.ra, r)
        return self

    def contract(self, dtype):
        """the same exchange by parallel/codec.py in ``dtype`` from this object's (unrun) inputs"""
        g, e, q = (t.cpu().to(dtype).clone() for t in (self.g, self.e, self.q))
        want, p = contract([(self.plan, slice(0, g.numel()))], [g], [e], qs := [q], [1.0], dtype)
        return {"P-hat": p, "Q": qs[0], "e": e, "g": want}


def contract(items, gl, res, qprev, weights, dtype):
    """One exchange by parallel/codec.py in ``dtype``: items = (plan, slice of the flat buffer) per bucket,
    gl = the ranks' gradients; res (per rank) and qprev (per bucket) are carried -> (decoded, last P-hat);
    outside the tables' rows the result keeps rank 0's gradient."""
    from ddlpc.parallel import codec as C
    want = gl[0].to(dtype).clone()
    for bi, (plan, sl) in enumerate(items):
        wp, wq = [], []
        for g, e, w in zip(gl, res, weights):
            wp.append(torch.zeros(plan.wire_p, dtype=dtype))
            C.powersgd_project(g[sl].to(dtype), e[sl], qprev[bi], wp[-1], plan, w)
        p = torch.stack(wp).sum(0)
        C.powersgd_orthonormalize(p, plan)
        for e, w in zip(res, weights):
            ql = torch.zeros(plan.wire_q, dtype=dtype)
            wq.append(torch.zeros_like(ql))
            C.powersgd_backproject(e[sl], p, ql, wq[-1], plan, w)
            C.powersgd_residual(e[sl], p, ql, plan)
        qprev[bi] = torch.stack(wq).sum(0)
        C.powersgd_decode(want[sl], p, qprev[bi], plan)
    return want, p


def assert_close(name, got, ref64, ref32):
    err, err32 = float((got.cpu().double() - ref64).norm()), float((ref32.double() - ref64).norm())
    bound = 8 * err32 + ulp32(float(ref64.abs().max()))
    print(f"powersgd {name}: kernel {err:.3e}, fp32 contract {err32:.3e}, bound {bound:.3e}")
    assert err <= bound, (name, err, bound)


def gauss(seed, scale=1.0):
    return lambda k: torch.randn(k, generator=_gen(seed)) * scale


def run_gaussian(o, dev, n=33, m=257, r=4):
    x = Exchange(o, dev, n, m, r, gauss(1, 1e-2), gauss(2, 1e-3), gauss(3))
    ref64, ref32 = x.contract(torch.float64), x.contract(torch.float32)
    x.run()
    for name, got in (("P-hat", x.wire_p), ("Q", x.wire_q), ("e", x.e), ("g", x.g)):
        assert_close(f"{dev} {name}", got, ref64[name], ref32[name])


def run_zero(o, dev):        # zero gradient, zero residual: zero columns, decode = +0, nothing non-finite
    x = Exchange(o, dev, 33, 257, 4, torch.zeros, torch.zeros, gauss(3)).run()
    for name in ("g", "e", "wire_p", "wire_q"):
        t = getattr(x, name)
        assert_bits(t, torch.zeros(t.numel()), name)


def run_refusal(o, dev):     # a low row that ends one float past g: refused on the host before any launch
    x = Exchange(o, dev, 17, 32, 4, gauss(1), gauss(2), gauss(3))
    off, n, m = (int(v) for v in x.plan.low[-1, :3])
    x.g, x.e = x.g[:off + n * m - 1], x.e[:off + n * m - 1]
    with pytest.raises(RuntimeError, match="points past a buffer"):
        x.run()


CASES = [(run_int, *c, shift) for c in INT_CASES for shift in (0, 3)] + [(run_orth_exact, r) for r in RS] + \
    [(run_zero,), (run_gaussian,), (run_refusal,)]
IDS = ["-".join([c[0].__name__[4:]] + [str(int(a)) for a in c[1:]]) for c in CASES]
