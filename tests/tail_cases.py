"""Exact cases for the gradient tail: the slab reduction + scatter every weight gradient leaves the
library through (``reduce_rows_scatter``, ``reduce_rows``), the direct-grad forms of every operator
that takes gradient outs, the transposed conv's bias gradient from statistics rows
(``colsum_rows=``) and the two scalars ``head_grad_scale`` / ``meter_add``.  Written once and run
on both kernel sets: ``test_tail_exact_gpu.py`` (``csrc/reduce.hip`` behind ``csrc/bindings.cpp``)
and its ``test_tail_exact_cpu.py`` mirror (``csrc/cpu_ref.cpp``).  docs/TESTING.md, "The gradient
tail", has the regime table, the defect table and what is not covered.

Slabs.  Every element is ``k 2^e`` with integer ``|k| <= 1023`` and integer ``e`` in [-8, 8]: exact
in fp32, and every partial sum of at most 4 097 of them is a multiple of 2^-8 below 2^31, so exact
in fp64 in ANY order.  The kernels accumulate in fp64 and round once, so the result must be
``float32(exact sum)`` bit for bit: the reference is ``slab.double().sum(0)`` on the CPU, permuted
by a written-out ``view / permute``.  ``slab_case`` asserts on the reference alone that the sum of
magnitudes per column stays below 2^44 (indeed below 2^31) and, from 64 rows up, that a sequential
fp32 accumulation of the same rows differs from the reference in at least 30 % of the columns, so
an fp32 accumulator anywhere in a regime fails its cases (``RECORD`` keeps the measured shares).
Cases of fewer than 16 columns take their columns from a larger pool, the first ones on which the
fp32 accumulation is wrong.

Accumulation.  ``accumulate=True`` is ``dst = dst + v`` in fp32 with ``v`` the fp32-rounded sum:
one IEEE addition per call, which has one correct result.  The reference is that addition done
twice on the CPU (``acc2``).  Where the data make ``prefill + 2 v`` exact in fp32 (the integer
gradients of the operator cases), ``check_direct`` asserts on the reference that both steps are
exact, so the expected value is ``prefill + 2 dW`` there; the slab cases, whose sums need more
than 24 bits, and a device scale of 0.3 are held to the two additions.

``RECORD`` collects the worst ``sum |x|`` and ``|result| / 2^24`` and the fp32 shares (records for
docs/TESTING.md, not tolerances).
"""
import functools

import torch

import exact_cases as xc
import head_cases as hc

RECORD = {"abs_sum": 0.0, "result": 0.0, "share": {}, "scale_share": {}}

GUARD = 31337.0       # around every destination view
SENT = -77.0          # prefill of an overwritten destination
BIG = 2.0 ** 20       # the unread columns of a strided slab
OFF = 5               # floats in front of a destination view: 20 bytes, off every 16-byte boundary


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bool(bad.any()):
        i = bad.nonzero()[:6].flatten().tolist()
        g, w = got.detach().cpu().flatten(), want.flatten()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first {i}: got "
                             f"{[float(g[j]) for j in i]} want {[float(w[j]) for j in i]}")


def guarded(n, dev, fill):
    """a view of n floats, OFF floats into a GUARD-filled allocation and 16-byte misaligned,
    prefilled with `fill` (a number or a CPU tensor) -> (allocation, view)"""
    buf = torch.full((OFF + n + 7,), GUARD, dtype=torch.float32, device=dev)
    view = buf[OFF:OFF + n]
    if isinstance(fill, torch.Tensor):
        view.copy_(fill.reshape(-1))
    else:
        view.fill_(fill)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return buf, view


def guards_intact(buf, n, what):
    b = buf.detach().cpu()
    assert bool((b[:OFF] == GUARD).all()) and bool((b[OFF + n:] == GUARD).all()), f"{what}: wrote outside its out"


def prefill(n):
    """small integers j in [-3, 3]"""
    return (torch.arange(n) % 7 - 3).float()


def acc2(pre, v):
    """dst = dst + v in fp32, twice (one correctly rounded addition per call)"""
    pre, v = pre.detach().cpu().float().reshape(-1), v.detach().cpu().float().reshape(-1)
    return (pre + v) + v


# ------------------------------------------------------------------ slabs
def slab_values(R, N, seed):
    g = _gen(seed)
    k = torch.randint(-1023, 1024, (R, N), generator=g).double()
    e = torch.randint(-8, 9, (R, N), generator=g).double()
    v = k * torch.pow(torch.tensor(2.0, dtype=torch.float64), e)
    assert torch.equal(v.float().double(), v)             # exact in fp32
    assert torch.equal((v * 256).round(), v * 256)        # multiples of 2^-8
    return v.float()


def seq_fp32(rows):
    """the sequential fp32 accumulation of the rows (what the kernels must NOT compute)"""
    acc = torch.zeros(rows.shape[1], dtype=torch.float32)
    for r in range(rows.shape[0]):
        acc = acc + rows[r]
    return acc


@functools.lru_cache(maxsize=2)
def slab_case(R, N, seed=None):
    """-> (values [R][N] fp32, exact fp64 column sums), the preconditions asserted"""
    seed = 1000 * R + N if seed is None else seed
    pool = N if N >= 16 else N + 32
    v = slab_values(R, pool, seed)
    exact = v.double().sum(0)
    if R >= 64:
        wrong = seq_fp32(v) != exact.float()
        if pool > N:                                       # the first N columns fp32 gets wrong
            cols = wrong.nonzero().flatten()[:N]
            assert cols.numel() == N, f"bad case R={R} N={N}: too few columns in the pool"
            v, exact, wrong = v[:, cols].contiguous(), exact[cols], wrong[cols]
        share = float(wrong.double().mean())
        RECORD["share"][(R, N)] = share
        assert share >= 0.30, f"bad case R={R} N={N}: fp32 accumulation differs in only {share:.2f} of the columns"
    else:
        v, exact = v[:, :N].contiguous(), exact[:N]
    mag = v.double().abs().sum(0)
    assert float(mag.max()) < 2.0 ** 31 < 2.0 ** 44       # every partial sum exact in fp64
    assert torch.equal(v.double().flip(0).sum(0), exact)   # (another order, the same sum)
    RECORD["abs_sum"] = max(RECORD["abs_sum"], float(mag.max()))
    RECORD["result"] = max(RECORD["result"], float(exact.abs().max()) / 2.0 ** 24)
    return v, exact


def permuted(sums, mode, T, B):
    """slab order -> destination order, written out: mode 0 [co][tap][ci] -> OIHW [co][ci][tap],
    mode 1 [ci][sub][co] -> IOHW [ci][co][sub], mode 2 identity"""
    if mode == 2:
        return sums
    A = sums.numel() // (T * B)
    return sums.view(A, T, B).permute(0, 2, 1).contiguous().view(-1)


def run_scatter(o, dev, c):
    """reduce_rows_scatter: overwrite into a sentinel-filled out, the same call again (same
    bits), accumulate twice into small integers; guards, and the slab unwritten"""
    R, N, mode, T, B, ld = c["R"], c["N"], c["mode"], c.get("T", 0), c.get("B", 0), c.get("ld", -1)
    if mode != 2:
        assert N == c["A"] * T * B
    v, exact = slab_case(R, N)
    ref = permuted(exact, mode, T, B).float()
    if ld > 0:                                             # [R][2][96]: the rows' other columns hold BIG
        assert ld == 192 and N <= 96
        slab = torch.full((R, 2, 96), BIG, dtype=torch.float32)
        slab[:, 0, :N] = v
    else:
        slab = v
    sd = slab.to(dev).contiguous()
    call = lambda dst, acc: o.reduce_rows_scatter(sd, R, N, dst, mode, T, B, acc, ld)
    what = f"R={R} N={N} mode={mode} ld={ld}"
    outs = []
    for _ in range(2):
        buf, dst = guarded(N, dev, SENT)
        assert call(dst, False) is None
        guards_intact(buf, N, what)
        outs.append(dst.clone())
    assert_bits(outs[0], ref, what + " overwrite")
    assert_bits(outs[1], outs[0].cpu(), what + " second call")
    pre = prefill(N)
    buf, dst = guarded(N, dev, pre)
    call(dst, True)
    call(dst, True)
    guards_intact(buf, N, what)
    assert_bits(dst, acc2(pre, ref), what + " accumulate twice")
    assert torch.equal(sd.cpu(), slab), what + ": the slab was written"


def run_reduce_rows(o, dev, R, N):
    """reduce_rows: the fp64 sums equal the exact sums; the same bits again; the slab unwritten"""
    v, exact = slab_case(R, N)
    sd = v.to(dev)
    got = o.reduce_rows(sd, R, N)
    assert got.dtype == torch.float64 and tuple(got.shape) == (N,)
    assert_bits(got, exact, f"reduce_rows R={R} N={N}")
    assert_bits(o.reduce_rows(sd, R, N), got.cpu(), f"reduce_rows R={R} N={N} second call")
    assert torch.equal(sd.cpu(), v)


# ------------------------------------------------------------------ direct grads
class Tap:
    """the operator namespace with one operator's calls recorded: (args, kwargs, result, path).
    The runners of exact_cases / head_cases build the operands, call the returning form and
    prove its gradient exact against fp64; the direct form is then called on the same operands."""

    def __init__(self, o, name):
        self._o, self._name, self.calls = o, name, []

    def __getattr__(self, k):
        f = getattr(self._o, k)
        if k != self._name:
            return f

        def tapped(*a, **kw):
            r = f(*a, **kw)
            self.calls.append((a, kw, r, self._o.last_path()))
            return r
        return tapped


def check_direct(got, pre, ret, what, q=None):
    """out == prefill + ret + ret in fp32; q: the case is exact — both additions are, the
    value is prefill + 2 ret, a multiple of q below 2^24 q (asserted on the reference alone)"""
    want = acc2(pre, ret)
    if q is not None:
        p, r = pre.double().reshape(-1), ret.detach().cpu().double().reshape(-1)
        assert torch.equal((p + r).float().double(), p + r) and torch.equal(want.double(), p + 2 * r), \
            f"{what}: bad case, prefill + 2 grad is not exact in fp32"
        m = (p + 2 * r) / q
        assert torch.equal(m, m.round()) and float(m.abs().max()) < xc.F32_EXACT, \
            f"{what}: bad case, prefill + 2 grad is not a multiple of q={q} below 2^24 q"
        RECORD["result"] = max(RECORD["result"], float(m.abs().max()) / 2.0 ** 24)
    assert_bits(got.reshape(-1), want, what)


def direct_outs(o, dev, call, rets, path, names, qs, adjacent=False):
    """call(outs) runs the direct form twice into prefilled guarded views, one per gradient in
    `rets` (adjacent: consecutive views of ONE allocation); asserts the accumulated values, the
    empty returns, the guards and the path"""
    sizes = [r.numel() for r in rets]
    pres = [prefill(n) + i for i, n in enumerate(sizes)]
    if adjacent:
        buf, flat = guarded(sum(sizes), dev, torch.cat(pres))
        views, at = [], 0
        for n in sizes:
            views.append(flat[at:at + n])
            at += n
        bufs = [(buf, sum(sizes))]
    else:
        pairs = [guarded(n, dev, p) for n, p in zip(sizes, pres)]
        views, bufs = [v for _, v in pairs], [(b, n) for (b, _), n in zip(pairs, sizes)]
    outs = [v.view(r.shape) for v, r in zip(views, rets)]
    for _ in range(2):
        empties = call(outs)
        assert o.last_path() == path, (o.last_path(), path)
        for e in empties:
            assert e.numel() == 0, "the direct form must return empty gradients"
    for b, n in bufs:
        guards_intact(b, n, names[0])
    for v, p, r, name, q in zip(views, pres, rets, names, qs):
        check_direct(v, p, r, name, q)


def _with(args, at, vals):
    a = list(args)
    for i, v in zip(at, vals):
        a[i] = v
    return a


def run_direct_conv3_wgrad(o, dev, c):
    """conv3_wgrad(out=): args[5]"""
    tap = Tap(o, "conv3_wgrad")
    xc.run_conv3_wgrad(tap, dev, c)
    a, kw, dW, path = tap.calls[0]
    q = (0.5 if c.get("pro") or c.get("pro2") else 1.0) * (0.125 if c.get("dypro") else 1.0)
    direct_outs(o, dev, lambda outs: [o.conv3_wgrad(*_with(a, [5], outs), **kw)], [dW], path, ["dW"], [q])
    assert torch.equal(o.conv3_wgrad(*a, **kw), dW)        # the returning form: the control
    return path


def run_direct_bwd32(o, dev, c):
    """conv3_bwd32(dw_out=): args[4] -> (path, slab rows = BN partial rows)"""
    tap = Tap(o, "conv3_bwd32")
    xc.run_conv3_bwd32(tap, dev, c)
    a, kw, (dA, part, dW), path = tap.calls[0]

    def call(outs):
        r = o.conv3_bwd32(*_with(a, [4], outs), **kw)
        assert torch.equal(r[0], dA) and torch.equal(r[1], part)
        return [r[2]]
    direct_outs(o, dev, call, [dW], path, ["dW"], [0.5])
    return path, part.shape[0]


def run_direct_convt(o, dev, c, fused):
    """convt_wgrad(dw_out=, db_out=): args[2], args[3]; convt_bwd_fused: args[3], args[4]"""
    name = "convt_bwd_fused" if fused else "convt_wgrad"
    tap = Tap(o, name)
    (xc.run_convt_bwd_fused if fused else xc.run_convt_wgrad)(tap, dev, c)
    a, kw, r, path = tap.calls[0]
    dW, db = r[-2], r[-1]
    at = [3, 4] if fused else [2, 3]

    def call(outs):
        g = getattr(o, name)(*_with(a, at, outs), **kw)
        if fused:
            assert torch.equal(g[0], r[0]) and torch.equal(g[1], r[1])
        return g[-2:]
    direct_outs(o, dev, call, [dW, db], path, ["dW", "db"], [0.5 if c.get("bn") else 1.0, 1.0])
    return path


def run_direct_head_bwd(o, dev, c):
    """head_ce_bwd(dw_out=, db_out=): args[7], args[8] (saturated integer case)"""
    tap = Tap(o, "head_ce_bwd")
    hc.run_bwd(tap, dev, c)
    a, kw, r, path = tap.calls[0]
    cs = hc.make(c)
    gs = hc._gscale(cs) / max(hc.reference(c, 1.0).count, 1)
    _, qW, _, _ = hc._q(cs, gs)

    def call(outs):
        g = o.head_ce_bwd(*_with(a, [7, 8], outs), **kw)
        assert torch.equal(g[0], r[0]) and torch.equal(g[3], r[3])
        return g[1:3]
    direct_outs(o, dev, call, [r[1], r[2]], path, ["dWh", "dbh"], [qW, abs(gs)])
    return path


def run_direct_head_bn_bwd(o, dev, c):
    """head_ce_bn_bwd(dgamma_out=, dbeta_out=): the outs come back as the returned tensors"""
    tap = Tap(o, "head_ce_bn_bwd")
    hc.run_bn_bwd(tap, dev, c)
    a, kw, (dY, dg, dbt), path = tap.calls[0]
    assert len(a) == 10 and not kw
    pres = [prefill(dg.numel()), prefill(dbt.numel()) + 1]
    pairs = [guarded(p.numel(), dev, p) for p in pres]
    for _ in range(2):
        g = o.head_ce_bn_bwd(*a, pairs[0][1], pairs[1][1])
        assert o.last_path() == path and torch.equal(g[0], dY)
        assert g[1].data_ptr() == pairs[0][1].data_ptr() and g[2].data_ptr() == pairs[1][1].data_ptr()
    for (buf, view), p, ret, name in zip(pairs, pres, (dg, dbt), ("dgamma", "dbeta")):
        guards_intact(buf, p.numel(), name)
        check_direct(view, p, ret, name)
    return path


def run_head_wgrad_from_rows(o, dev, c, scale, adjacent):
    """head_wgrad_from_rows on the rows of head_ce_fwd_stats (unit gradient scale, proven exact
    by head_cases): float32(float64(sum) * float64(scale)), returned and accumulated twice"""
    tap = Tap(o, "head_ce_fwd_stats")
    hc.run_fwd_stats(tap, dev, c)
    _, _, (out3, wrows, brows), _ = tap.calls[0]
    cs = hc.make(c)
    K, C = cs.K, cs.C
    sc = torch.tensor([scale], dtype=torch.float32)
    sums = wrows.detach().cpu().double().sum(0)
    mag = wrows.detach().cpu().double().abs().sum(0)
    m = sums / 0.5
    assert torch.equal(m, m.round()) and float((mag / 0.5).max()) < xc.F32_EXACT   # exact sums, 25 bits
    prod = sums * sc.double()                              # 25 x 24 bits: exact in fp64
    ref = prod.float()
    before = wrows.clone()
    dw, db = o.head_wgrad_from_rows(wrows, sc.to(dev), K, C)
    assert tuple(dw.shape) == (K, C) and tuple(db.shape) == (K,)
    assert_bits(dw.reshape(-1), ref[:K * C], "dWh")
    assert_bits(db, ref[K * C:], "dbh")
    path = o.last_path()
    q = 0.25 if scale == 0.5 else None                     # (0.3: the two additions round)
    direct_outs(o, dev, lambda outs: o.head_wgrad_from_rows(wrows, sc.to(dev), K, C, outs[0], outs[1]),
                [dw, db], path, ["dWh", "dbh"], [q, q], adjacent=adjacent)
    assert torch.equal(wrows, before)
    return wrows.shape[0]


def run_head_wgrad_synthetic(o, dev, R, K, C, scale, adjacent):
    """head_wgrad_from_rows on slab rows whose sums need up to 40 bits: the device scale must
    multiply the fp64 sum (one IEEE fp64 product, one rounding to fp32).  On the operator's own
    rows (sums below 2^24 quanta) a kernel that rounds the sum to fp32 first gives the same bits;
    from 64 rows up it differs in a share of the columns that is asserted on the reference alone."""
    N = K * C + K
    v, exact = slab_case(R, N)
    sc = torch.tensor([scale], dtype=torch.float32)
    ref = (exact * sc.double()).float()
    early = exact.float() * sc                             # (the sum rounded to fp32 first)
    share = float((early != ref).double().mean())
    RECORD["scale_share"][R] = share
    if R >= 64:                                            # (a few rows: the sums mostly fit fp32)
        assert share >= 0.10, f"bad case: scaling in fp32 differs in only {share:.2f} of the columns"
    rows = v.to(dev)
    dw, db = o.head_wgrad_from_rows(rows, sc.to(dev), K, C)
    assert_bits(dw.reshape(-1), ref[:K * C], "dWh")
    assert_bits(db, ref[K * C:], "dbh")
    direct_outs(o, dev, lambda outs: o.head_wgrad_from_rows(rows, sc.to(dev), K, C, outs[0], outs[1]),
                [dw, db], o.last_path(), ["dWh", "dbh"], [None, None], adjacent=adjacent)
    assert torch.equal(rows.cpu(), v)


# ------------------------------------------------------------------ colsum_rows
def run_colsum(o, dev, c, fused=False):
    """the transposed conv's bias gradient from the statistics rows [R][2][Ctot] of the concat
    data gradient that produced dUp (its first co1 channels): equal to the fp64 channel sums, to
    the channel_sum path and, accumulated twice, to the db_out= form
    -> (dgrad path, convT path)"""
    sp, Cf, Cdy, co1 = xc._shape(c), c["Cin"], c["Cout"], c["co1"]
    seed, d = c.get("seed", 2), c.get("dens", 0.5)
    w = xc.tern((Cdy, Cf, 3, 3), d, seed).float()
    dy = xc.tern(sp + (Cdy,), d, seed + 1)
    pk = xc.pack(o, w, dev)
    dUp, dSkip, rows = o.conv3_fwd(dy.to(dev), None, pk.dgrad, None, None, None, Cf, co1, True)
    dpath = o.last_path()
    ref = xc.dgrad_ref(dy.double(), w.double())
    xc.assert_exact(dUp, ref[..., :co1], "dUp")
    assert rows.dim() == 3 and rows.shape[1] == 2 and rows.shape[2] == Cf and co1 < Cf
    rc = rows.detach().cpu()
    # a wrong row stride, half or column offset must not pass by reading zeros
    assert int(torch.count_nonzero(rc[:, 0, co1:])) > 0, "bad case: the columns >= C are all zero"
    if not dpath.startswith("conv3_fwd:res:v7"):           # (v7 documents a sum^2 half of zeros)
        assert int(torch.count_nonzero(rc[:, 1, :])) > 0, "bad case: the sum^2 half is all zero"
    s, sa = xc.rows_ref(ref[..., :co1])
    assert int(torch.count_nonzero(s)) >= co1 // 2, "bad case: most channel sums are zero"
    Cx = 64
    x = xc.tern((sp[0], sp[1] // 2, sp[2] // 2, Cx), 0.5, seed + 7).to(dev)
    if fused:
        wt = xc.tern((Cx, co1, 2, 2), 0.5, seed + 8).float()
        wd = xc.pack(o, wt, dev).dgrad
        fn = lambda *r, **kw: o.convt_bwd_fused(x, dUp, wd, *r, **kw)[-2:]
    else:
        fn = lambda *r, **kw: o.convt_wgrad(x, dUp, *r, **kw)
    dW, db = fn(None, None, rows)
    path = o.last_path()
    xc.assert_exact(db, s, "db from colsum_rows", "f32", 1.0, sa)
    dW0, db0 = fn(None, None, None)                        # the channel_sum path
    assert o.last_path() == path
    assert_bits(db0, db.cpu(), "db: channel_sum path against colsum_rows")
    assert_bits(dW0, dW.cpu(), "dW")
    direct_outs(o, dev, lambda outs: fn(outs[0], outs[1], rows), [dW, db], path, ["dW", "db"], [1.0, 1.0])
    direct_outs(o, dev, lambda outs: fn(outs[0], outs[1], None), [dW, db], path, ["dW", "db (channel_sum)"],
                [1.0, 1.0])
    return dpath, path


# ------------------------------------------------------------------ the scalars
def run_head_grad_scale(o, dev, cnt, gs):
    """head_grad_scale = gs / count as one fp32 division; a count <= 0 divides by 1"""
    out3 = torch.tensor([0.75, 3.0, float(cnt)], dtype=torch.float32)
    g32 = torch.tensor([1.0 if gs is None else gs], dtype=torch.float32)
    want = g32 / torch.tensor([float(cnt) if cnt > 0 else 1.0], dtype=torch.float32)
    got = o.head_grad_scale(out3.to(dev), None if gs is None else g32.to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (1,)
    assert_bits(got, want, f"head_grad_scale count={cnt} gs={gs}")


def run_meter_add(o, dev):
    """five meter_add calls: buf == the Python-double running sums; loss32 * n is exact in fp64
    (24 bits x 6), so a fused multiply-add cannot change it; slots 4.. of the allocation untouched"""
    store = torch.full((8,), GUARD, dtype=torch.float64, device=dev)
    buf = store[:4]
    buf.zero_()
    want = [0.0, 0.0, 0.0, 0.0]
    ns = [1, 3, 50, 1, 3]
    for i in range(5):
        loss = torch.tensor([0.1 * (i + 1)], dtype=torch.float32)
        correct = torch.tensor([1000.0 + 17 * i], dtype=torch.float32)
        pixels, n = 4096.25 * (i + 1), ns[i]
        o.meter_add(buf, loss.to(dev), correct.to(dev), pixels, float(n))
        want[0] += float(loss[0]) * n
        want[1] += float(correct[0])
        want[2] += pixels
        want[3] += n
        assert store[:4].tolist() == want, (i, store[:4].tolist(), want)
    assert store[4:].tolist() == [GUARD] * 4
