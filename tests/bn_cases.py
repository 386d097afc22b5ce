"""Exact cases for the BatchNorm kernels (apply + pool, backward with pool routing, groups,
statistics / finalize, running statistics), written once and run on both kernel sets:
``test_bn_exact_gpu.py`` (the gfx950 kernels of ``csrc/bn.hip`` / ``csrc/reduce.hip``) and its
``test_bn_exact_cpu.py`` mirror (``csrc/cpu_ref.cpp``).

The method is that of ``exact_cases.py``.  On ternary ``y`` with the ``bn_stats4`` constants the
activation ``relu(y scale + shift)`` takes the six values 0, 0.5, 1, 1.5, 2, 3: exact in bf16, and
a large share of the pooling windows has a TIED positive maximum, so every such window pins the
first-maximum-wins routing of the pooled gradient.  ``dA`` and ``dP`` are ternary too, so every sum
the backward forms (sum dyh, sum dyh xhat) is a small multiple of 1/8: exact in fp32 in any order.

The routing reference is written out here (``route``): the first maximum in (kd, kh, kw) scan
order gets ``dP``, and the ReLU mask is the strict ``y scale + shift > 0``.  No ``max_pool``
indices are used.  Its preconditions are asserted on the reference alone for every pooled case:
at least 15 % of the (window, channel) pairs have a tied positive maximum and at least 5 % have
such a tie with the first maximum not at scan position 0.

dY divides by the pixel count, so it is held per element (``assert_bound``) to the fp64 formula
``k (dyh - m1 - xhat m2)``; a misrouted ``dP`` moves an element by at least ``|k| gs >= 0.25``,
orders of magnitude above the bound.

``WORST`` collects, per family, the worst observed error / bound of the bounded quantities
(records for docs/TESTING.md, not tolerances) and ``TIES`` the tie shares of the pooled cases.
"""
import math

import torch

from exact_cases import (assert_bound, assert_exact, bn_stats4, bnb_terms, ops, tern)  # noqa: F401

WORST = {}            # family -> worst |got - ref| / bound
TIES = {}             # case id -> (tied share, tied with first maximum not at 0)

GAMMAS = (0.5, 1.0, 2.0, -1.0)
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))      # the kernels take eps as fp32


def gamma_of(C):
    return torch.tensor(GAMMAS).repeat((C + 3) // 4)[:C].contiguous()


# ------------------------------------------------------------------ pooling windows, routing
def windows(x):
    """channel-last [N, (D,) H, W, C] -> [N, (Do,) Ho, Wo, C, K] with the window's K = 4 (8)
    pixels in (kd, kh, kw) scan order"""
    if x.dim() == 4:
        N, H, W, C = x.shape
        return x.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(
            N, H // 2, W // 2, C, 4)
    N, D, H, W, C = x.shape
    return x.reshape(N, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(
        N, D // 2, H // 2, W // 2, C, 8)


def unwindows(w, shape):
    """inverse of windows()"""
    if len(shape) == 4:
        N, H, W, C = shape
        return w.reshape(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(shape)
    N, D, H, W, C = shape
    return w.reshape(N, D // 2, H // 2, W // 2, C, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(shape)


def route(a64, dP64=None):
    """first-maximum-wins max-pool of the activation a64 and the routing of dP64:
    -> (pooled, unpooled dP or None, tied share, tied-and-first-not-at-0 share)"""
    w = windows(a64)
    K = w.shape[-1]
    mx = w.max(-1).values
    idx = torch.arange(K)
    ismax = w == mx[..., None]
    first = torch.where(ismax, idx, torch.tensor(K)).min(-1).values
    tied = (ismax.sum(-1) >= 2) & (mx > 0)
    un = None
    if dP64 is not None:
        onehot = (idx == first[..., None]).double()
        un = unwindows(onehot * dP64[..., None], tuple(a64.shape))
    return mx, un, float(tied.double().mean()), float((tied & (first > 0)).double().mean())


def assert_ties(tie, nf, what):
    assert tie >= 0.15, f"{what}: bad case, only {tie:.3f} of the windows have a tied positive maximum"
    assert nf >= 0.05, f"{what}: bad case, only {nf:.3f} tied with the first maximum not at position 0"
    TIES[what] = (tie, nf)


def _per_image(s4, G, N, r, ndim):
    """row r of stats4 [4][C] / [G][4][C] broadcast over a channel-last batch of G groups"""
    s = s4.double().reshape(G, 4, -1)[:, r]
    return s.repeat_interleave(N // G, 0).reshape(N, *([1] * (ndim - 2)), -1)


def act_of(y, s4, G=1):
    """relu(y scale + shift) in fp64 with each group's constants (exact, a bf16 value)"""
    yd = y.double()
    a = yd * _per_image(s4, G, y.shape[0], 2, y.dim()) + _per_image(s4, G, y.shape[0], 3, y.dim())
    return torch.relu(a)


def stats_of(C, seed, G=1):
    if G == 1:
        return bn_stats4(C, seed)
    return torch.stack([bn_stats4(C, seed + 7 * g) for g in range(G)]).contiguous()


def pooled_shape(shape):
    return (shape[0],) + tuple(s // 2 for s in shape[1:-1]) + (shape[-1],)


def record(fam, got, ref, bound):
    """worst |got - ref| / bound of a bounded quantity, then the assertion"""
    g, ref, bound = got.detach().double().cpu(), ref.double(), bound.double()
    err = (g - ref).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.tensor(math.inf), torch.tensor(0.0)))
    WORST[fam] = max(WORST.get(fam, 0.0), float(ratio.max()))
    bad = err > bound
    assert not bool(bad.any()), (f"{fam}: {int(bad.sum())} of {bad.numel()} outside the bound, first "
                                 f"{bad.nonzero()[:4].tolist()}, worst ratio {float(ratio.max()):.3f}")


def record_bound(fam, got, ref64, S64):
    """assert_bound plus the record of the worst ratio against its bound"""
    g = got.detach().double().cpu()
    b = 2.0 ** -8 * ref64.abs() + 2.0 ** -20 * S64
    err = (g - ref64).abs()
    ok = b > 0
    if bool(ok.any()):
        WORST[fam] = max(WORST.get(fam, 0.0), float((err[ok] / b[ok]).max()))
    assert_bound(got, ref64, S64, fam)


# ------------------------------------------------------------------ launch arithmetic (csrc/bn.hip)
def bn_bwd_reduce_blocks(items):
    return max(1, min((items + 63) // 64, 2048))


def bn_group_bwd_rows(items, groups):
    return max(1, min((items + 255) // 256, max(1, 4096 // groups)))


def v2_ok(shape, pool):
    G8 = shape[-1] // 8
    return shape[-1] % 8 == 0 and G8 & (G8 - 1) == 0 and G8 <= 256 and (
        not pool or all(s % 2 == 0 for s in shape[1:-1]))


def bwd_trips(shape, pool, groups=1):
    """(reduce trips, apply trips) of the grid-stride loops of the backward kernels for one
    group's tensor `shape`, restated from the launchers: v2 (bn_bwd2_kernel) walks UNROLL units
    per trip, unit = pixel or window; v1 (bn_bwd_kernel) one item per thread group per trip"""
    G8 = shape[-1] // 8
    pix = math.prod(shape[:-1])
    items = pix // (2 ** (len(shape) - 2)) if pool else pix
    nb = bn_bwd_reduce_blocks(items) if groups == 1 else bn_group_bwd_rows(items, groups)
    if v2_ok(shape, pool):
        kwin = pool and G8 > 32
        upb = 256 // (2 * G8 if pool and not kwin else G8)
        unroll = 1 if kwin and len(shape) == 5 else 2
        grid2 = max(1, min((items + 2 * upb - 1) // (2 * upb), max(1, 8192 // groups)))
        return (math.ceil(items / (unroll * nb * upb)), math.ceil(items / (unroll * grid2 * upb)))
    per = (256 // G8)                               # items per block per trip
    grid = max(1, min((items + max(1, per) - 1) // max(1, per), 2048))
    return math.ceil(items / (nb * per)), math.ceil(items / (grid * per))


def bn_group_stats_rows(gpix, C, groups):
    """partial rows (workgroups) per group of bn_group_finalize's statistics pass"""
    nb = (gpix * (C // 8) + 256 * 16 - 1) // (256 * 16)
    nb = min(nb, max(1, 4096 // groups))
    return max(1, min(nb, 256))


# ------------------------------------------------------------------ backward
def split_rows(total64, R, q, seed):
    """[C] totals (multiples of q) -> [R][C] fp32 rows of multiples of q that sum to them"""
    g = torch.Generator().manual_seed(seed)
    rows = (torch.randint(-3, 4, (R, total64.numel()), generator=g).double() + (total64 / q / R).floor()) * q
    rows[-1] = total64 - rows[:-1].sum(0)
    assert float(rows.abs().max()) / q < 2 ** 24
    assert torch.equal(rows.float().double(), rows)
    return rows.float()


def backward_ref(y, dA, dP, s4, gamma, G, gs, what):
    """fp64 reference of bn_backward / bn_group_backward: per-group sums [G][2][C], their
    sums of magnitudes, dY and its bound magnitude S"""
    N, C = y.shape[0], y.shape[-1]
    dt = dA.double() if dA is not None else torch.zeros(y.shape, dtype=torch.float64)
    if dP is not None:
        _, un, tie, nf = route(act_of(y, s4, G), dP.double())
        assert_ties(tie, nf, what)
        dt = dt + un
    dyh, xh = bnb_terms(dt * gs, y, s4, G)
    cnt = y[..., 0].numel() // G
    d3, x3 = dyh.reshape(G, -1, C), (dyh * xh).reshape(G, -1, C)
    sums = torch.stack([d3.sum(1), x3.sum(1)], 1)                    # [G][2][C]
    mags = torch.stack([d3.abs().sum(1), x3.abs().sum(1)], 1)
    k = gamma.double() * s4.double().reshape(G, 4, C)[:, 1]          # [G][C]
    m = sums / cnt

    def img(v):
        return v.repeat_interleave(N // G, 0).reshape(N, *([1] * (y.dim() - 2)), C)
    ref = img(k) * (dyh - img(m[:, 0]) - xh * img(m[:, 1]))
    S = img(k).abs() * (dyh.abs() + img(m[:, 0]).abs() + xh.abs() * img(m[:, 1]).abs())
    return sums, mags, k, m, ref, S


def run_backward(o, dev, c):
    """bn_backward (groups = 1) / bn_group_backward: dgamma / dbeta exact (also accumulated into
    pre-filled outs), dY per element; rows=R feeds the partial rows instead of the reduction"""
    shape, G, pool = tuple(c["shape"]), c.get("groups", 1), bool(c.get("pool"))
    C, seed, what = shape[-1], c.get("seed", 11), c["id"]
    use_a = c.get("dA", True)
    gs = 0.5 if c.get("gscale") else 1.0
    y = tern(shape, 0.5, seed)
    dA = tern(shape, 0.5, seed + 1) if use_a else None
    dP = tern(pooled_shape(shape), 0.5, seed + 2) if pool else None
    s4, gamma = stats_of(C, seed + 3, G), gamma_of(C)
    sums, mags, k, m, ref, S = backward_ref(y, dA, dP, s4, gamma, G, gs, what)
    if "trips" in c:
        per_group = (shape[0] // G,) + shape[1:]
        assert bwd_trips(per_group, pool, G) == tuple(c["trips"]), (what, bwd_trips(per_group, pool, G))
    t = lambda v: None if v is None else v.to(dev)
    pre = c.get("prefill")
    dg0 = torch.arange(C, dtype=torch.float32) % 7 - 3 if pre else None
    db0 = torch.arange(C, dtype=torch.float32) % 5 - 2 if pre else None
    dgo, dbo = (dg0.clone().to(dev), db0.clone().to(dev)) if pre else (None, None)
    part = None
    if c.get("rows"):
        R = c["rows"]
        rows = torch.stack([torch.stack([split_rows(sums[g, 0], R, 0.125, seed + 20 + g),
                                         split_rows(sums[g, 1], R, 0.125, seed + 40 + g)], 1)
                            for g in range(G)])                      # [G][R][2][C]
        part = rows.reshape(G * R, 2, C).contiguous().to(dev)
    if G == 1 and not c.get("group_op"):
        gsc = torch.tensor([0.5], device=dev) if c.get("gscale") else None
        dY, dg, db = o.bn_backward(t(dA), t(dP), t(y), t(s4), t(gamma), gsc, dgo, dbo, part)
    else:
        dY, dg, db = o.bn_group_backward(t(dA), t(dP), t(y), t(s4), t(gamma), G, dgo, dbo, part)
    path = o.last_path()
    fam = "bn_group_backward" if (G > 1 or c.get("group_op")) else "bn_backward"
    dgr, dbr = sums[:, 1].sum(0), sums[:, 0].sum(0)
    if pre:
        assert dg.data_ptr() == dgo.data_ptr() and db.data_ptr() == dbo.data_ptr()
        dgr, dbr = dgr + dg0.double(), dbr + db0.double()
    assert_exact(dg, dgr, "dgamma", "rows", 0.125, mags[:, 1].sum(0) + 4, fam)
    assert_exact(db, dbr, "dbeta", "rows", 0.125, mags[:, 0].sum(0) + 4, fam)
    record_bound(fam + " dY", dY, ref, S)
    return path


def run_backward_big(o, dev, shape, pool, seed=17):
    """bn_backward above the apply pass's grid cap (8 192 workgroups): one call, the fp64
    reference formed image by image; dgamma / dbeta exact, dY per element over every element"""
    N, C = shape[0], shape[-1]
    y, dA = tern(shape, 0.5, seed), tern(shape, 0.5, seed + 1)
    dP = tern(pooled_shape(shape), 0.5, seed + 2) if pool else None
    s4, gamma = stats_of(C, seed + 3), gamma_of(C)
    t = lambda v: None if v is None else v.to(dev)
    dY, dg, db = o.bn_backward(t(dA), t(dP), t(y), t(s4), t(gamma), None)
    path = o.last_path()
    sums, mags = torch.zeros(2, C, dtype=torch.float64), torch.zeros(2, C, dtype=torch.float64)
    terms, ties = [], []
    for n in range(N):
        yi = y[n:n + 1]
        dt = dA[n:n + 1].double()
        if pool:
            _, un, tie, nf = route(act_of(yi, s4), dP[n:n + 1].double())
            ties.append((tie, nf))
            dt = dt + un
        dyh, xh = bnb_terms(dt, yi, s4)
        for r, v in enumerate((dyh, dyh * xh)):
            sums[r] += v.reshape(-1, C).sum(0)
            mags[r] += v.abs().reshape(-1, C).sum(0)
        terms.append((dyh.float(), xh.float()))            # small multiples of 1/2: exact in fp32
    if pool:
        assert_ties(min(a for a, _ in ties), min(b for _, b in ties), f"big pooled {shape}")
    assert_exact(dg, sums[1], "dgamma", "rows", 0.125, mags[1], "bn_backward")
    assert_exact(db, sums[0], "dbeta", "rows", 0.125, mags[0], "bn_backward")
    cnt = y[..., 0].numel()
    k, m1, m2 = gamma.double() * s4[1].double(), sums[0] / cnt, sums[1] / cnt
    for n in range(N):
        dyh, xh = terms[n][0].double(), terms[n][1].double()
        ref = k * (dyh - m1 - xh * m2)
        S = k.abs() * (dyh.abs() + m1.abs() + xh.abs() * m2.abs())
        record_bound("bn_backward dY", dY[n:n + 1], ref, S)
    return path


def grad_coefs_inputs(c):
    """-> y, stats4, gamma, the fp64 reference (sums, magnitudes, k, m), the integer rows [R][2][C]
    and the pre-filled outs"""
    shape, C, seed, R = tuple(c["shape"]), c["shape"][-1], c.get("seed", 12), c["rows"]
    y, dA = tern(shape, 0.5, seed), tern(shape, 0.5, seed + 1)
    s4, gamma = stats_of(C, seed + 3), gamma_of(C)
    sums, mags, k, m, _, _ = backward_ref(y, dA, None, s4, gamma, 1, 1.0, c["id"])
    part = torch.stack([split_rows(sums[0, 0], R, 0.125, seed + 20),
                        split_rows(sums[0, 1], R, 0.125, seed + 40)], 1).contiguous()     # [R][2][C]
    pre = c.get("prefill")
    dg0 = (torch.arange(C, dtype=torch.float32) % 7 - 3) if pre else None
    db0 = (torch.arange(C, dtype=torch.float32) % 5 - 2) if pre else None
    return y, s4, gamma, sums, mags, k, m, part, pre, dg0, db0


def run_grad_coefs(o, dev, c):
    """bn_grad_coefs from integer rows: k bit-equal, m1 / m2 the fp64 quotient rounded once"""
    C = c["shape"][-1]
    y, s4, gamma, sums, mags, k, m, part, pre, dg0, db0 = grad_coefs_inputs(c)
    t = lambda v: None if v is None else v.to(dev)
    coefs, dg, db = o.bn_grad_coefs(part.to(dev), y.to(dev), s4.to(dev), gamma.to(dev),
                                     dg0.clone().to(dev) if pre else None, db0.clone().to(dev) if pre else None)
    path = o.last_path()
    want = torch.stack([k[0].float(), m[0, 0].float(), m[0, 1].float()])
    assert coefs.dtype == torch.float32 and torch.equal(coefs.cpu(), want), (
        "coefs", (coefs.cpu() != want).nonzero()[:8].tolist())
    dgr, dbr = sums[0, 1], sums[0, 0]
    if pre:
        dgr, dbr = dgr + dg0.double(), dbr + db0.double()
    assert_exact(dg, dgr, "dgamma", "rows", 0.125, mags[0, 1] + 4, "bn_grad_coefs")
    assert_exact(db, dbr, "dbeta", "rows", 0.125, mags[0, 0] + 4, "bn_grad_coefs")
    return path


# ------------------------------------------------------------------ forward apply
def run_apply(o, dev, c):
    """bn_relu_apply / bn_group_apply, bit-exact: the activation and the window maximum of the
    stored bf16 activations"""
    shape, G, pool = tuple(c["shape"]), c.get("groups", 1), bool(c.get("pool"))
    full, seed, C = c.get("full", True), c.get("seed", 13), c["shape"][-1]
    y = tern(shape, 0.5, seed)
    s4 = stats_of(C, seed + 3, G)
    a64 = act_of(y, s4, G)
    if G > 1 or c.get("group_op"):
        a, p = o.bn_group_apply(y.to(dev), s4.to(dev), G, pool)
        fam = "bn_group_apply"
    else:
        a, p = o.bn_relu_apply(y.to(dev), s4.to(dev), pool, full)
        fam = "bn_relu_apply"
    path = o.last_path()
    if full:
        assert_exact(a, a64, "activation", q=0.5, family=fam)
    else:
        assert a.numel() == 0
    if pool:
        mx, _, tie, nf = route(a64)
        assert_ties(tie, nf, c["id"])
        assert_exact(p, mx, "pooled", q=0.5, family=fam)
    else:
        assert p.numel() == 0
    return path


# ------------------------------------------------------------------ statistics / finalize
def finalize_ref(A, B, count, gamma, beta):
    """the kernels' formula in fp64 from exact sums A = sum y, B = sum y^2 ([..., C]):
    -> dict of references and bounds (see docs/TESTING.md for the derivation)"""
    A, B, g, b = A.double(), B.double(), gamma.double(), beta.double()
    mean = A / count
    var = (B / count - mean * mean).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + EPS32)
    sc = g * inv
    unb = var * count / (count - 1) if count > 1 else var
    return dict(mean=mean, var=var, inv=inv, scale=sc, shift=b - mean * sc, unb=unb,
                shift_bound=2.0 ** -22 * (b.abs() + (mean * sc).abs()))


def check_stats4(fam, st, r):
    st = st.detach().cpu()
    assert st.dtype == torch.float32
    want = r["mean"].float()
    assert torch.equal(st[..., 0, :], want), (fam + " mean", (st[..., 0, :] != want).nonzero()[:8].tolist())
    record(fam + " invstd", st[..., 1, :], r["inv"], 2.0 ** -23 * r["inv"].abs())
    record(fam + " scale", st[..., 2, :], r["scale"], 2.0 ** -22 * r["scale"].abs())
    record(fam + " shift", st[..., 3, :], r["shift"], r["shift_bound"])


def finalize_rows_case(P, C, count, seed):
    """synthetic exact sums of `count` virtual pixels per channel, split into P integer rows.
    Edge channels: 0 constant (y = 3: var = 0), 1 negative variance (B lowered below A^2 / count:
    the clamp), 2 and 3 cancellation (y = 64 + ternary), the rest ternary"""
    yv = tern((count, C), 0.5, seed).double()
    yv[:, 0] = 3.0
    yv[:, 2:4] += 64.0
    A, B = yv.sum(0), (yv * yv).sum(0)
    if count > 1:
        A[1] = float(max(2, count // 2 + 1))
        B[1] = float(int(A[1]) ** 2 // count)
        if int(A[1]) ** 2 % count == 0:
            B[1] -= 1
        assert float(B[1] / count - (A[1] / count) ** 2) < 0
    g = torch.Generator().manual_seed(seed + 1)
    rows = torch.randint(-3, 4, (P, 2, C), generator=g).double()
    rows[:, 0] += (A / P).floor()
    rows[:, 1] += (B / P).floor()
    rows[-1, 0] = A - rows[:-1, 0].sum(0)
    rows[-1, 1] = B - rows[:-1, 1].sum(0)
    assert float(rows.abs().max()) < 2 ** 24 and torch.equal(rows.float().double(), rows)
    assert torch.equal(rows[:, 0].sum(0), A) and torch.equal(rows[:, 1].sum(0), B)
    return rows.float().contiguous(), A, B


def finalize_inputs(c):
    """-> rows [P][2][C], their exact sums A, B, gamma, beta, the running statistics before"""
    P, C, count, seed = c["P"], c["C"], c["count"], c.get("seed", 14)
    rows, A, B = finalize_rows_case(P, C, count, seed)
    g = torch.Generator().manual_seed(seed + 2)
    gamma, beta = gamma_of(C), torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return rows, A, B, gamma, beta, rm0, rv0


def run_finalize(o, dev, c):
    """bn_finalize from integer rows [P][2][C]: stats4 and the running statistics (nbt + 1)"""
    count = c["count"]
    rows, A, B, gamma, beta, rm0, rv0 = finalize_inputs(c)
    mom = 0.1
    m32 = float(torch.tensor(mom, dtype=torch.float32))
    r = finalize_ref(A, B, count, gamma, beta)
    if count > 1:
        assert float(r["var"][0]) == 0.0 and float(r["var"][1]) == 0.0     # constant / clamped
        assert abs(float(r["inv"][0]) - 1.0 / math.sqrt(EPS32)) < 1e-9
    rm, rv = rm0.clone().to(dev), rv0.clone().to(dev)
    nbt = torch.tensor(5, dtype=torch.int64, device=dev)
    st = o.bn_finalize(rows.to(dev), float(count), gamma.to(dev), beta.to(dev), rm, rv, mom, EPS, True, nbt)
    path = o.last_path()
    check_stats4("bn_finalize", st, r)
    for name, got, x, r0 in (("mean", rm, r["mean"], rm0.double()), ("var", rv, r["unb"], rv0.double())):
        record("bn_finalize running " + name, got, m32 * x + (1 - m32) * r0,
               2.0 ** -22 * ((m32 * x).abs() + ((1 - m32) * r0).abs()))
    assert int(nbt) == 6
    rm2, rv2 = rm0.clone().to(dev), rv0.clone().to(dev)
    st2 = o.bn_finalize(rows.to(dev), float(count), gamma.to(dev), beta.to(dev), rm2, rv2, mom, EPS, False, nbt)
    assert torch.equal(st2, st) and torch.equal(rm2.cpu(), rm0) and torch.equal(rv2.cpu(), rv0)
    assert int(nbt) == 6
    return path


SENTINEL = -77.0


def group_finalize_inputs(c):
    """-> y, groups, C, seed, gamma, beta, pixels per group, the exact per-group sums A, B"""
    shape, G, seed = tuple(c["shape"]), c["groups"], c.get("seed", 15)
    C = shape[-1]
    y = tern(shape, 0.5, seed)
    y[..., 2:4] += 64
    y[..., 0] = 2                                                      # a constant channel
    gen = torch.Generator().manual_seed(seed + 1)
    gamma, beta = gamma_of(C), torch.randn(C, generator=gen)
    yd = y.double().reshape(G, -1, C)
    return y, G, C, seed, gamma, beta, yd.shape[1], yd.sum(1), (yd * yd).sum(1)


def group_rows(A, B, G, R, seed):
    """the exact per-group sums split into R integer rows each: [G * R][2][C]"""
    rows = torch.stack([torch.stack([split_rows(A[g], R, 1.0, seed + 20 + g),
                                     split_rows(B[g], R, 1.0, seed + 40 + g)], 1) for g in range(G)])
    return rows.reshape(G * R, 2, -1).contiguous()


def run_group_finalize(o, dev, c):
    """bn_group_finalize on ternary y (channels 2 and 3 offset by 64: cancellation) and
    bn_group_finalize_rows on the exact per-group rows: stats4, and the arena rows at aoff = 16"""
    y, G, C, seed, gamma, beta, count, A, B = group_finalize_inputs(c)
    # the kernel's fp32 partial rows are exact: a workgroup sums about count / nb pixels
    nb = bn_group_stats_rows(count, C, G)
    assert nb == c.get("nb", nb), (c["id"], nb)
    assert float(B.max()) / count * (math.ceil(count / nb) + 256) < 2 ** 24
    r = finalize_ref(A, B, count, gamma, beta)
    aoff, cols = 16, 16 + 2 * C + 24
    arena = torch.full((G + 1, cols), SENTINEL).to(dev)
    st = o.bn_group_finalize(y.to(dev), G, gamma.to(dev), beta.to(dev), EPS, arena, aoff)

    def check(fam, st, arena):
        assert tuple(st.shape) == (G, 4, C)
        check_stats4(fam, st, r)
        ar = arena.cpu()
        keep = torch.ones_like(ar, dtype=torch.bool)
        keep[:G, aoff:aoff + 2 * C] = False
        assert bool((ar[keep] == SENTINEL).all()), fam + ": arena written outside [aoff, aoff + 2C) x groups"
        assert torch.equal(ar[:G, aoff:aoff + C], r["mean"].float()), fam + " arena mean"
        record(fam + " arena var", ar[:G, aoff + C:aoff + 2 * C], r["unb"], 2.0 ** -23 * r["unb"].abs())
    check("bn_group_finalize", st, arena)
    arena2 = torch.full((G + 1, cols), SENTINEL).to(dev)
    st2 = o.bn_group_finalize_rows(group_rows(A, B, G, 3, seed).to(dev), G, float(count),
                                   gamma.to(dev), beta.to(dev), EPS, arena2, aoff)
    check("bn_group_finalize_rows", st2, arena2)
    assert torch.equal(st2, st) and torch.equal(arena2, arena), "finalize_rows differs from finalize"
    return count


# ------------------------------------------------------------------ running statistics
def running_ref(r0, slots, m32, exact):
    """K momentum updates in fp64, in slot order; exact: every term representable in fp32"""
    r = r0.double()
    for k in range(slots.shape[0]):
        a, b = m32 * slots[k].double(), (1 - m32) * r
        r = a + b
        if exact:
            for v in (a, b, r):
                assert torch.equal(v.float().double(), v), "bad case: a step is not exact in fp32"
    return r


def running_case(Cs, K, exact, seed):
    """per layer: running mean / var inside a sentinel-padded buffer, K arena rows of slots"""
    g = torch.Generator().manual_seed(seed)
    offs, o_ = [], 8
    for C in Cs:
        offs.append(o_)
        o_ += 2 * C + 8                                               # sentinel columns between layers
    cols = o_
    if exact:
        arena = torch.randint(-16, 17, (K + 1, cols), generator=g).float() / 4
        bufs = [torch.randint(-4, 5, (2 * C + 16,), generator=g).float() for C in Cs]
    else:
        arena = torch.randn(K + 1, cols, generator=g)
        bufs = [torch.randn(2 * C + 16, generator=g).abs() + 0.1 for C in Cs]
    return offs, arena, bufs


def running_call(o, dev, c, mom, offs, arena0, bufs0):
    """the operator call of run_running on copies of the case on `dev` -> arena, buffers, nbts, layers"""
    Cs, K = c["Cs"], c["K"]
    arena = arena0.clone().to(dev)
    bufs = [b.clone().to(dev) for b in bufs0]
    # running_mean at [4, 4 + C), running_var at [C + 12, 2C + 12) of the padded buffer
    rms = [b[4:4 + C] for b, C in zip(bufs, Cs)]
    rvs = [b[C + 12:2 * C + 12] for b, C in zip(bufs, Cs)]
    nbts = [torch.tensor(3, dtype=torch.int64, device=dev) for _ in Cs]
    layers = list(range(len(Cs)))
    if c.get("all"):
        layers = layers[:-1]                                          # the last layer stays out
        rows = [[rms[i].data_ptr(), rvs[i].data_ptr(), nbts[i].data_ptr(), Cs[i] | (offs[i] << 32)]
                for i in layers]
        entries = torch.tensor(rows, dtype=torch.int64).to(dev)
        o.bn_running_apply_all(entries, arena, K, max(Cs[i] for i in layers), mom)
    else:
        for i in layers:
            o.bn_running_apply(rms[i], rvs[i], arena[:K, offs[i]:offs[i] + 2 * Cs[i]], mom, nbts[i])
    return arena, bufs, nbts, layers


def run_running(o, dev, c):
    """bn_running_apply (per layer, a column slice of the arena) or bn_running_apply_all (entries
    built as fused_unet.py's bn_defer_apply does): K in-order updates, nbt += K, and nothing else
    written"""
    Cs, K, exact, seed = c["Cs"], c["K"], c["exact"], c.get("seed", 16)
    mom = 0.25 if exact else 0.1
    m32 = float(torch.tensor(mom, dtype=torch.float32))
    offs, arena0, bufs0 = running_case(Cs, K, exact, seed)
    arena, bufs, nbts, layers = running_call(o, dev, c, mom, offs, arena0, bufs0)
    assert torch.equal(arena.cpu(), arena0), "the arena was written"
    fam = "bn_running_apply_all" if c.get("all") else "bn_running_apply"
    for i, C in enumerate(Cs):
        b, b0 = bufs[i].cpu(), bufs0[i]
        if i not in layers:
            assert torch.equal(b, b0) and int(nbts[i]) == 3, "a layer outside entries was touched"
            continue
        assert int(nbts[i]) == 3 + K
        pad = torch.ones_like(b0, dtype=torch.bool)
        pad[4:4 + C] = False
        pad[C + 12:2 * C + 12] = False
        assert torch.equal(b[pad], b0[pad]), "written outside the running buffers"
        for lo, col in ((4, offs[i]), (C + 12, offs[i] + C)):
            slots = arena0[:K, col:col + C]
            ref = running_ref(b0[lo:lo + C], slots, m32, exact)
            if exact:
                assert torch.equal(b[lo:lo + C].double(), ref), fam + ": exact case differs"
            else:
                mag = torch.maximum(b0[lo:lo + C].abs(), slots.abs().max(0).values).double()
                record(fam, b[lo:lo + C], ref, K * 2.0 ** -22 * mag)
    return fam


# ------------------------------------------------------------------ the two backends agree
def assert_same(what, gpu, cpu):
    """the GPU operator's results and the CPU operator's, bit for bit"""
    assert len(gpu) == len(cpu)
    for i, (g, h) in enumerate(zip(gpu, cpu)):
        assert g.dtype == h.dtype and g.shape == h.shape, (what, i, g.dtype, h.dtype, g.shape, h.shape)
        ne = g.cpu() != h
        assert not bool(ne.any()), f"{what}: result {i} differs in {int(ne.sum())} of {ne.numel()} elements"


def agree_finalize(o, c):
    rows, _, _, gamma, beta, rm0, rv0 = finalize_inputs(c)

    def call(dev):
        rm, rv = rm0.clone().to(dev), rv0.clone().to(dev)
        nbt = torch.tensor(5, dtype=torch.int64, device=dev)
        st = o.bn_finalize(rows.to(dev), float(c["count"]), gamma.to(dev), beta.to(dev), rm, rv, 0.1, EPS, True, nbt)
        return st, rm, rv, nbt
    assert_same("bn_finalize " + c["id"], call("cuda"), call("cpu"))


def agree_group_finalize(o, c):
    y, G, C, seed, gamma, beta, count, A, B = group_finalize_inputs(c)
    rows = group_rows(A, B, G, 3, seed)

    def call(dev):
        ar, ar2 = (torch.full((G + 1, 16 + 2 * C + 24), SENTINEL).to(dev) for _ in range(2))
        st = o.bn_group_finalize(y.to(dev), G, gamma.to(dev), beta.to(dev), EPS, ar, 16)
        st2 = o.bn_group_finalize_rows(rows.to(dev), G, float(count), gamma.to(dev), beta.to(dev), EPS, ar2, 16)
        return st, ar, st2, ar2
    assert_same("bn_group_finalize " + c["id"], call("cuda"), call("cpu"))


def agree_running(o, c):
    assert not c["exact"]
    offs, arena0, bufs0 = running_case(c["Cs"], c["K"], False, c.get("seed", 16))

    def call(dev):
        _, bufs, nbts, _ = running_call(o, dev, c, 0.1, offs, arena0, bufs0)
        return bufs + nbts
    assert_same("running statistics " + c["id"], call("cuda"), call("cpu"))


def agree_grad_coefs(o, c):
    y, s4, gamma, _, _, _, _, part, pre, dg0, db0 = grad_coefs_inputs(c)

    def call(dev):
        return o.bn_grad_coefs(part.to(dev), y.to(dev), s4.to(dev), gamma.to(dev),
                               dg0.clone().to(dev) if pre else None, db0.clone().to(dev) if pre else None)
    assert_same("bn_grad_coefs " + c["id"], call("cuda"), call("cpu"))


def agree_group_backward_rows(o, c):
    """dgamma / dbeta of bn_group_backward from precomputed rows: the per-group fp64 sums added in
    group order on both backends (rows whose sum over the groups depends on the order).  The
    per-group coefficients are not an output of the operator, so they are not compared here
    (docs/TESTING.md); dY is held per element by run_backward"""
    shape, G, R, seed = tuple(c["shape"]), c["groups"], c["rows"], c.get("seed", 11)
    C = shape[-1]
    y, dA = tern(shape, 0.5, seed), tern(shape, 0.5, seed + 1)
    s4, gamma = stats_of(C, seed + 3, G), gamma_of(C)
    # Within a group the rows are of like magnitude, so their fp64 sum is exact in any order.
    # Across the groups it is not: group 1 is minus group 0 at 2^70 times group 2's size, so
    # (g0 + g1) + g2 = g2 in group order and 0 in the orders that add g2 to a large term first.
    assert G == 3
    gen = torch.Generator().manual_seed(seed + 5)
    part = (torch.randn(G, R, 2, C, generator=gen) * 1e3).float()
    part[0] *= 2.0 ** 70
    part[1] = -part[0]
    gs = part.double().sum(1)                                          # [G][2][C], exact
    assert bool((((gs[0] + gs[1]) + gs[2]).float() != ((gs[0] + gs[2]) + gs[1]).float()).all()), "bad case"
    part = part.reshape(G * R, 2, C).contiguous()
    dg0, db0 = torch.arange(C, dtype=torch.float32) % 7 - 3, torch.arange(C, dtype=torch.float32) % 5 - 2

    def call(dev):
        out = []
        for pre in (False, True):
            dgo, dbo = (dg0.clone().to(dev), db0.clone().to(dev)) if pre else (None, None)
            _, dg, db = o.bn_group_backward(dA.to(dev), None, y.to(dev), s4.to(dev), gamma.to(dev), G, dgo, dbo,
                                            part.to(dev))
            out += [dg, db]
        return out
    assert_same("bn_group_backward rows " + c["id"], call("cuda"), call("cpu"))


# ------------------------------------------------------------------ bindings
CROSS_DEVICE = "on the host"          # (names with it need a second device: skipped on the CPU)


def _binding_args(dev):
    """valid arguments of every BatchNorm / tail operator at C = 8, two images of 4 x 4 pixels"""
    C = 8
    f = lambda *s, dt=torch.float32, d=dev: torch.zeros(*s, dtype=dt, device=d)
    return dict(
        C=C, f=f, y=f(2, 4, 4, C, dt=torch.bfloat16), dA=f(2, 4, 4, C, dt=torch.bfloat16),
        dP=f(2, 2, 2, C, dt=torch.bfloat16), part=f(3, 2, C), gamma=f(C) + 1, beta=f(C), s4=f(4, C) + 1,
        s4g=f(2, 4, C) + 1, rm=f(C), rv=f(C) + 1, nbt=f(1, dt=torch.int64)[0], arena=f(3, 2 * C + 8),
        entries=f(0, 4, dt=torch.int64))


def binding_accepts(o, dev):
    """the valid neighbours of binding_calls: every operator runs on the shared arguments"""
    a = _binding_args(dev)
    C, f = a["C"], a["f"]
    st = o.bn_finalize(a["part"], 32.0, a["gamma"], a["beta"], a["rm"], a["rv"], 0.1, EPS, True, a["nbt"])
    assert tuple(st.shape) == (4, C) and int(a["nbt"]) == 1
    o.bn_running_apply(a["rm"], a["rv"], a["arena"][:2, 4:4 + 2 * C], 0.1, a["nbt"])
    assert int(a["nbt"]) == 3
    o.bn_running_apply_all(a["entries"], a["arena"], 2, C, 0.1)
    o.bn_relu_apply(a["y"], a["s4"], True, True)
    o.bn_group_apply(a["y"], a["s4g"], 2, True)
    o.bn_backward(a["dA"], a["dP"], a["y"], a["s4"], a["gamma"], None, f(C), f(C), None)
    o.bn_backward(a["dA"], None, a["y"], a["s4"], a["gamma"], None, None, None, a["part"])
    o.bn_group_backward(a["dA"], None, a["y"], a["s4g"], a["gamma"], 2, None, None, f(6, 2, C))
    # an empty partial means "no rows given": the operator reduces dA itself, as without one
    want = o.bn_group_backward(a["dA"] + 1, None, a["y"], a["s4g"], a["gamma"], 2, None, None, None)
    got = o.bn_group_backward(a["dA"] + 1, None, a["y"], a["s4g"], a["gamma"], 2, None, None, f(0))
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and bool((want[2] != 0).any())
    o.bn_grad_coefs(a["part"], a["y"], a["s4"], a["gamma"], f(C), f(C))
    o.bn_group_finalize(a["y"], 2, a["gamma"], a["beta"], EPS, a["arena"], 8)
    o.bn_group_finalize_rows(f(6, 2, C), 2, 16.0, a["gamma"], a["beta"], EPS, a["arena"], 8)
    assert float(o.reduce_rows(f(3 * 5) + 1, 3, 5)[4]) == 3.0


def binding_calls(o, dev):
    """name -> a call both registrations must refuse (csrc/tail_checks.h) before any launch: one
    call per check the operators gained"""
    a = _binding_args(dev)
    C, f = a["C"], a["f"]
    y, dA, dP, part, gamma, beta, s4, s4g, rm, rv, nbt, arena = (a[k] for k in (
        "y", "dA", "dP", "part", "gamma", "beta", "s4", "s4g", "rm", "rv", "nbt", "arena"))
    strided = lambda: f(2 * C)[::2]
    fin = lambda p=part, g=gamma, b=beta, m=rm, v=rv, n=nbt, upd=True: o.bn_finalize(
        p, 32.0, g, b, m, v, 0.1, EPS, upd, n)
    run = lambda m=rm, v=rv, s=None, n=nbt: o.bn_running_apply(
        m, v, arena[:2, 4:4 + 2 * C] if s is None else s, 0.1, n)
    bwd = lambda dA=dA, dP=None, s4=s4, g=gamma, dg=None, db=None, p=None, gs=None: o.bn_backward(
        dA, dP, y, s4, g, gs, dg, db, p)
    gbwd = lambda s4=s4g, g=gamma, G=2, p=None, dP=None: o.bn_group_backward(dA, dP, y, s4, g, G, None, None, p)
    coefs = lambda p=part, s4=s4, g=gamma, dg=None, db=None: o.bn_grad_coefs(p, y, s4, g, dg, db)
    gfin = lambda G=2, g=gamma, b=beta, ar=arena, off=8: o.bn_group_finalize(y, G, g, b, EPS, ar, off)
    gfr = lambda p=None, G=2, g=gamma, b=beta, ar=arena, off=8: o.bn_group_finalize_rows(
        f(6, 2, C) if p is None else p, G, 16.0, g, b, EPS, ar, off)
    return {
        "bn_finalize partial not a multiple of 2C": lambda: fin(p=f(3 * 2 * C - 1)),
        "bn_finalize partial fp64": lambda: fin(p=part.double()),
        "bn_finalize beta shorter": lambda: fin(b=f(C - 1)),
        "bn_finalize beta fp64": lambda: fin(b=beta.double()),
        "bn_finalize beta on the host": lambda: fin(b=f(C, d="cpu")),
        "bn_finalize running_mean shorter": lambda: fin(m=f(C - 1)),
        "bn_finalize running_mean fp64": lambda: fin(m=rm.double()),
        "bn_finalize running_mean strided": lambda: fin(m=strided()),
        "bn_finalize running_mean on the host": lambda: fin(m=f(C, d="cpu")),
        "bn_finalize running_var longer": lambda: fin(v=f(C + 1)),
        "bn_finalize running_var strided": lambda: fin(v=strided()),
        "bn_finalize running_var shorter, no update": lambda: fin(v=f(C - 1), upd=False),
        "bn_finalize nbt int32": lambda: fin(n=nbt.int()),
        "bn_finalize nbt on the host": lambda: fin(n=f(1, dt=torch.int64, d="cpu")[0]),
        "bn_running_apply running_var shorter": lambda: run(v=f(C - 1)),
        "bn_running_apply running_mean fp64": lambda: run(m=rm.double()),
        "bn_running_apply running_mean strided": lambda: run(m=strided()),
        "bn_running_apply slots narrower": lambda: run(s=arena[:2, 4:4 + 2 * C - 1]),
        "bn_running_apply slots column stride": lambda: run(s=f(2, 4 * C)[:, ::2]),
        "bn_running_apply slots on the host": lambda: run(s=f(2, 2 * C, d="cpu")),
        "bn_running_apply nbt int32": lambda: run(n=nbt.int()),
        "bn_running_apply_all entries int32": lambda: o.bn_running_apply_all(f(0, 4, dt=torch.int32), arena, 2, C, 0.1),
        "bn_running_apply_all entries [L][3]": lambda: o.bn_running_apply_all(f(1, 3, dt=torch.int64), arena, 2, C, 0.1),
        "bn_running_apply_all fewer arena rows than K": lambda: o.bn_running_apply_all(a["entries"], arena, 4, C, 0.1),
        "bn_running_apply_all maxC wider than the arena": lambda: o.bn_running_apply_all(a["entries"], arena, 2, C + 5, 0.1),
        "bn_running_apply_all arena fp64": lambda: o.bn_running_apply_all(a["entries"], arena.double(), 2, C, 0.1),
        "bn_relu_apply stats4 shorter": lambda: o.bn_relu_apply(y, f(3, C), True, True),
        "bn_relu_apply stats4 fp64": lambda: o.bn_relu_apply(y, s4.double(), True, True),
        "bn_relu_apply stats4 on the host": lambda: o.bn_relu_apply(y, f(4, C, d="cpu"), True, True),
        "bn_relu_apply neither output": lambda: o.bn_relu_apply(y, s4, False, False),
        "bn_group_apply stats4 of one group": lambda: o.bn_group_apply(y, s4, 2, True),
        "bn_group_apply groups not dividing": lambda: o.bn_group_apply(y, f(3, 4, C), 3, True),
        "bn_backward stats4 shorter": lambda: bwd(s4=f(3, C)),
        "bn_backward gamma shorter": lambda: bwd(g=f(C - 1)),
        "bn_backward gamma fp64": lambda: bwd(g=gamma.double()),
        "bn_backward dA of another size": lambda: bwd(dA=f(2, 4, 3, C, dt=torch.bfloat16)),
        "bn_backward dP of another size": lambda: bwd(dP=f(2, 2, 3, C, dt=torch.bfloat16)),
        "bn_backward neither dA nor dP": lambda: bwd(dA=None),
        "bn_backward dgamma_out alone": lambda: bwd(dg=f(C)),
        "bn_backward dbeta_out shorter": lambda: bwd(dg=f(C), db=f(C - 1)),
        "bn_backward dgamma_out strided": lambda: bwd(dg=strided(), db=f(C)),
        "bn_backward partial not a multiple of 2C": lambda: bwd(p=f(2 * C + 1)),
        "bn_backward partial with dP": lambda: bwd(dP=dP, p=part),
        "bn_backward partial with gscale": lambda: bwd(p=part, gs=f(1) + 1),
        "bn_backward gscale fp64": lambda: bwd(gs=f(1, dt=torch.float64) + 1),
        "bn_group_backward stats4 of one group": lambda: gbwd(s4=s4),
        "bn_group_backward groups 0": lambda: gbwd(G=0),
        "bn_group_backward gamma shorter": lambda: gbwd(g=f(C - 1)),
        "bn_group_backward partial not a multiple of groups 2C": lambda: gbwd(p=f(3, 2, C)),
        "bn_grad_coefs partial not a multiple of 2C": lambda: coefs(p=f(3 * 2 * C - 1)),
        "bn_grad_coefs no rows": lambda: coefs(p=f(0)),
        "bn_grad_coefs stats4 shorter": lambda: coefs(s4=f(3, C)),
        "bn_grad_coefs gamma longer": lambda: coefs(g=f(C + 1)),
        "bn_grad_coefs dbeta_out alone": lambda: coefs(db=f(C)),
        "bn_grad_coefs stats4 on the host": lambda: coefs(s4=f(4, C, d="cpu")),
        "bn_group_finalize gamma shorter": lambda: gfin(g=f(C - 1)),
        "bn_group_finalize beta fp64": lambda: gfin(b=beta.double()),
        "bn_group_finalize groups not dividing": lambda: gfin(G=3),
        "bn_group_finalize arena narrower than aoff + 2C": lambda: gfin(off=9),
        "bn_group_finalize fewer arena rows than groups": lambda: gfin(ar=arena[:1]),
        "bn_group_finalize aoff negative": lambda: gfin(off=-1),
        "bn_group_finalize arena on the host": lambda: gfin(ar=f(3, 2 * C + 8, d="cpu")),
        "bn_group_finalize_rows partial not a multiple of groups 2C": lambda: gfr(p=f(3, 2, C)),
        "bn_group_finalize_rows beta shorter": lambda: gfr(b=f(C - 1)),
        "bn_group_finalize_rows groups 0": lambda: gfr(G=0),
        "bn_group_finalize_rows arena narrower than aoff + 2C": lambda: gfr(off=9),
        "reduce_rows partial shorter than R x N": lambda: o.reduce_rows(f(14), 3, 5),
        "reduce_rows partial fp64": lambda: o.reduce_rows(f(15, dt=torch.float64), 3, 5),
    }


BINDING_NAMES = list(binding_calls(None, "cpu"))      # (the calls are built lazily: none runs here)
