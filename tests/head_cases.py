"""Exact and per-element cases for the 1x1 head / cross-entropy operators, written once and run
on both kernel sets: ``test_head_exact_gpu.py`` (``csrc/head_ce.hip``) and its
``test_head_exact_cpu.py`` mirror (``csrc/cpu_ref.cpp``).  docs/TESTING.md, "Head and
cross-entropy", has the method, the bound derivation and the worst figures.

Saturated integer cases ("sat").  Softmax is not linear but it saturates exactly: with ternary
activations, head weights ``128 K tern`` (``256 K tern`` behind the deferred BatchNorm, whose
activations are multiples of 1/2) and biases ``128 pi(k)`` (pi a permutation) the logits of a
pixel are pairwise distinct multiples of 128.  exp(-128) underflows to 0 in fp32 however it is
evaluated, so ``se = 1``, the softmax is exactly one-hot, ``lse = m``, and every output is an
exact small-integer expression of the inputs: ``xc.assert_exact`` (bit equality with the fp64
reference after checking the precondition on the reference alone).  ``sat_precondition`` adds
the head's own conditions: every top-2 gap >= 128, >= 40 % of the valid pixels with a non-zero
gradient, >= 10 % hits.

Gaussian cases ("gauss"): fp64 reference from the bf16 / fp32 values and the per-element
bounds of ``bounds()``; ``RATIO`` records the worst error / bound per family.

Tie cases ("tie"): the integer construction with two identical weight rows and biases.  The
logits are still exact integers, so count and hits are exact against the FIRST maximum; the
(1/2, 1/2) softmax goes through rcp(2) and is held to the Gaussian bounds.

Worst figures over the cases of ``test_head_exact_gpu.py`` (``xc.WORST`` / ``RATIO`` collect
them while the cases run).  Saturated, max|ref| / q: bf16 outputs 64 (bound 256), rows
1 879 552 (bound 2^24), logits 898.  Gaussian, worst error / bound on the CPU / gfx950
kernels: logits 0.031 / 0.031; dA 0.96 / 0.96 (the bf16 store; its fp32 part over eps S:
0.0003 / 0.031); dWh 0.004 / 0.007; dbh 0.0001 / 0.003; BN partial rows 0.052 / 0.053; loss
0.0007 / 0.007; dY 0.96 / 0.96 (the bf16 store); dgamma, dbeta 0.04 / 0.04.
"""
import functools
import math

import torch

import exact_cases as xc

RATIO = {}           # family -> worst error / bound seen by check_bound (docs; not a tolerance)


# ------------------------------------------------------------------ inputs (CPU, seeded)
class Case:
    pass


def _key(c):
    return tuple(sorted(c.items()))


@functools.lru_cache(maxsize=3)
def _make(key):
    c = dict(key)
    mode, N, H, W, C, K = c["mode"], c["N"], c["H"], c["W"], c["C"], c["K"]
    defer, G, seed = bool(c.get("defer")), max(c.get("groups", 0), 1), c.get("seed", 7)
    ign = c.get("ignore_index", -100)
    P = N * H * W
    g = torch.Generator().manual_seed(seed)
    cs = Case()
    cs.c, cs.P, cs.C, cs.K, cs.G, cs.defer, cs.ign, cs.mode = c, P, C, K, G, defer, ign, mode
    integer = mode in ("sat", "tie")
    if integer:
        cs.y = xc.tern((N, H, W, C), 0.6, seed)
    else:
        cs.y = (torch.randn((N, H, W, C), generator=g) * (1.5 if defer else 1.0) + (0.3 if defer else 0.0)).bfloat16()
    cs.s4 = None
    if defer:     # exact-constant BatchNorm in both modes: a different set of constants per group
        cs.s4 = (torch.stack([xc.bn_stats4(C, seed + 10 + i) for i in range(G)]).contiguous() if G > 1
                 else xc.bn_stats4(C, seed + 3))
    if integer:
        wscale = 256.0 if defer else 128.0
        cs.Wh = (wscale * K * xc.tern((K, C), 0.5, seed + 1).float()).contiguous()
        cs.bh = 128.0 * torch.randperm(K, generator=g).float()
        if mode == "tie":
            k1, k2 = c["tie"]
            assert k1 < k2 < K
            cs.Wh[k2] = cs.Wh[k1]
            cs.bh[k2] = cs.bh[k1]
    else:
        sp = c["spread"]
        cs.Wh = (sp * torch.randn((K, C), generator=g)).contiguous()
        cs.bh = 0.3 * sp * torch.randn((K,), generator=g)
    # labels: a share follows the reference arg-max (hits), the rest is uniform
    z = _act(cs) @ cs.Wh.double().t() + cs.bh.double()
    am = _first_max(z)
    lab = torch.randint(0, K, (P,), generator=g)
    u = torch.rand((P,), generator=g)
    lab = torch.where(u < 0.15, am, lab)
    if mode == "tie":     # the later of the tied classes as label wherever the tie wins: a
        k1, k2 = c["tie"]  # last-maximum arg-max would count those pixels as hits
        lab = torch.where((am == k1) & (u > 0.6), torch.full_like(lab, k2), lab)
    # ignored pixels
    igm = torch.zeros(P, dtype=torch.bool)
    what = c.get("ignored", "pow2" if integer else "some")
    if what == "all":
        igm[:] = True
    else:
        if c.get("lead"):
            igm[:c["lead"]] = True
        if what == "pow2":           # valid count = the largest power of two <= 3/4 of the rest
            rest = (~igm).nonzero().flatten()
            keep = 2 ** int(math.floor(math.log2(max(1.0, 0.75 * rest.numel()))))
            perm = rest[torch.randperm(rest.numel(), generator=g)]
            igm[perm[keep:]] = True
        elif what == "some":
            igm |= torch.rand((P,), generator=g) < 0.03
    cs.lab = torch.where(igm, torch.full_like(lab, ign), lab).reshape(N, H, W).contiguous()
    cs.gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)] if integer \
        else torch.rand((C,), generator=g) + 0.5
    return cs


def make(c):
    return _make(_key(c))


def _rows(cs, r):
    """row r of the BatchNorm constants per pixel: [P][C] fp64"""
    s = cs.s4.double().reshape(cs.G, 4, cs.C)
    gi = torch.arange(cs.P) // (cs.P // cs.G)
    return s[gi, r]


def _act(cs):
    """the head's input activation [P][C] in fp64: the bf16 tensor, or bf16(relu(y scale + shift))
    (y scale + shift is exact in fp64 and the kernels form it with one fma, so the single
    rounding to fp32 and the rounding to bf16 are reproduced by the two casts)"""
    y = cs.y.double().reshape(-1, cs.C)
    if not cs.defer:
        return y
    pre = y * _rows(cs, 2) + _rows(cs, 3)
    return torch.relu(pre.float().bfloat16().double())


def _first_max(z):
    K = z.shape[1]
    m = z.max(1, keepdim=True).values
    return torch.where(z == m, torch.arange(K).expand_as(z), torch.full_like(z, K, dtype=torch.long)).min(1).values


# ------------------------------------------------------------------ fp64 reference
class Ref:
    pass


@functools.lru_cache(maxsize=3)
def _reference(key, gs):
    cs = _make(key)
    P, C, K = cs.P, cs.C, cs.K
    r = Ref()
    W, b = cs.Wh.double(), cs.bh.double()
    r.A = _act(cs)
    r.z = r.A @ W.t() + b
    r.L = (r.A.abs() @ W.abs().t() + b.abs()).max(1).values
    r.Lk = r.A.abs() @ W.abs().t() + b.abs()
    if K > 1:
        top = r.z.topk(2, dim=1).values
        r.gap = top[:, 0] - top[:, 1]
    else:
        r.gap = torch.full((P,), float("inf"), dtype=torch.float64)
    r.am = _first_max(r.z)
    lab = cs.lab.reshape(-1)
    r.valid = lab != cs.ign
    labc = torch.where(r.valid, lab, torch.zeros_like(lab))
    onehot = torch.nn.functional.one_hot(labc, K).double()
    # softmax as fp32 can hold it: a term exp(z - m) below the smallest fp32 denormal is 0
    # (the saturated regime rests on this; elsewhere it moves p by less than 2^-149)
    m = r.z.max(1, keepdim=True).values
    e = torch.exp(r.z - m)
    e = torch.where(e < 2.0 ** -149, torch.zeros_like(e), e)
    se = e.sum(1, keepdim=True)
    p = e / se
    r.lse = (m + torch.log(se))[:, 0]
    vz = r.valid.double()
    r.loss_px = (r.lse - r.z.gather(1, labc[:, None])[:, 0]) * vz
    r.count = int(r.valid.sum())
    r.hit = (r.am == lab)
    r.hits = int(r.hit.sum())
    r.loss = float(r.loss_px.sum()) / max(r.count, 1)
    r.d = (p - onehot) * gs * vz[:, None]
    r.D = (p + onehot) * abs(gs) * vz[:, None]
    r.dA = r.d @ W
    r.S = r.D @ W.abs()
    r.eps = 2.0 ** -15 * (1 + r.L)
    r.dW = r.d.t() @ r.A
    r.db = r.d.sum(0)
    if cs.defer:
        pre = cs.y.double().reshape(-1, C) * _rows(cs, 2) + _rows(cs, 3)
        r.mask = pre > 0
        r.dyh = torch.where(r.mask, r.dA, torch.zeros_like(r.dA))
        r.xh = (cs.y.double().reshape(-1, C) - _rows(cs, 0)) * _rows(cs, 1)
    return r


def reference(c, gs):
    return _reference(_key(c), float(gs))


def sat_precondition(cs, r):
    """the saturated regime, asserted on the reference alone"""
    if cs.K > 1:
        assert float(r.gap.min()) >= 128, f"bad case: top-2 gap {float(r.gap.min())} < 128"
    if cs.K == 1:       # one class: loss 0, every gradient 0, every valid pixel a hit
        assert float(r.loss_px.abs().max()) == 0 and r.hits == r.count
        assert float(r.dA.abs().max()) == 0 and float(r.dW.abs().max()) == 0
    if r.count and cs.K > 1:
        nz = int((r.valid & (r.am != cs.lab.reshape(-1))).sum())
        assert nz >= 0.4 * r.count, f"bad case: {nz} of {r.count} valid pixels have a gradient"
        assert r.hits >= 0.1 * r.count, f"bad case: {r.hits} hits of {r.count}"


# ------------------------------------------------------------------ assertions
def check_bound(got, ref, bound, what, fam):
    """|got - ref| <= bound per element (exact equality where the bound is 0)"""
    g = got.detach().double().cpu().reshape(ref.shape)
    err = (g - ref).abs()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite values"
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    RATIO[fam] = max(RATIO.get(fam, 0.0), ratio)
    bad = err > bound
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements exceed the bound; first "
                             f"{i}: got {float(g[i])!r} ref {float(ref[i])!r} bound {float(bound[i])!r}; "
                             f"worst error / bound {ratio:.3g}")


def _n_wg(cs, rows):
    """(an upper estimate of) the largest pixel count one workgroup accumulates"""
    return -(-cs.P // max(rows, 1)) + 256


def bounds(cs, r, rows, rounded):
    """per-element / per-row bounds of docs/TESTING.md for one case.  rounded: the BatchNorm
    partials are formed from the stored (bf16) dA, else from the unrounded fp32 one."""
    b = Ref()
    n_wg = _n_wg(cs, rows)
    acc = n_wg * 2.0 ** -24
    e = r.eps[:, None]
    b.dA = 2.0 ** -8 * r.dA.abs() + e * r.S
    b.dW = (e * r.D).t() @ r.A.abs() + acc * (r.d.abs().t() @ r.A.abs())    # sum of eps |a_c| D_k
    b.db = (e * r.D).sum(0) + acc * r.d.abs().sum(0)
    b.loss = (2.0 ** -16 * (1 + r.L) + 2.0 ** -22 * r.lse.abs()) * r.valid.double()
    b.loss_sum = b.loss.sum() + acc * r.loss_px.abs().sum()
    if cs.defer:
        m = r.mask.double()
        edA = ((2.0 ** -8 * r.dA.abs() if rounded else 0.0) + e * r.S) * m
        b.edyh = edA
        G = cs.G
        t1, t2 = r.dyh.reshape(G, -1, cs.C), (r.dyh * r.xh).reshape(G, -1, cs.C)
        b.p1 = edA.reshape(G, -1, cs.C).sum(1) + acc * t1.abs().sum(1)
        b.p2 = (edA * r.xh.abs()).reshape(G, -1, cs.C).sum(1) + acc * t2.abs().sum(1)
    return b


def check_hits(cs, r, out3, exact):
    cnt, hits = float(out3[2]), float(out3[1])
    assert cnt == r.count, (cnt, r.count)
    if exact:
        assert hits == r.hits, f"hits {hits} != {r.hits} (first-maximum reference)"
        return
    amb = r.valid & (r.gap < 2.0 ** -14 * (1 + r.L))
    assert int(amb.sum()) <= 0.001 * r.count, f"bad case: {int(amb.sum())} ambiguous pixels"
    lo, hi = r.hits - int((amb & r.hit).sum()), r.hits + int((amb & ~r.hit).sum())
    assert lo <= hits <= hi, (lo, hits, hi)


def check_loss(cs, r, out3, exact, b=None, fam=None):
    got = out3.detach().cpu()
    if exact:
        # the exact sums divided in fp64 and rounded once: what ce_finalize computes
        want = torch.tensor(r.loss_px.sum().item() / max(r.count, 1), dtype=torch.float64).float()
        assert r.loss_px.abs().sum() < xc.F32_EXACT * 128
        assert float(got[0]) == float(want), (float(got[0]), float(want))
    else:
        ref = torch.tensor([r.loss_px.sum().item()])
        bound = b.loss_sum.reshape(1) + 2.0 ** -23 * ref.abs()
        check_bound(got[0:1].double() * r.count, ref, bound, "loss sum", fam + ".loss")


def _dev(cs, dev):
    t = lambda v: None if v is None else v.to(dev)
    return t(cs.y), t(cs.Wh), t(cs.bh), t(cs.lab), t(cs.s4)


def _out3(r, dev):
    return torch.tensor([r.loss, float(r.hits), float(r.count)], dtype=torch.float32, device=dev)


def _gscale(cs):
    return 0.5 if cs.mode != "gauss" else 0.75


def _q(cs, gs):
    """quanta of the saturated regime: (dA, dW rows, partial rows) as multiples of"""
    half = 0.5 if cs.defer else 1.0
    return 128.0 * abs(gs), half * abs(gs), 128.0 * abs(gs), 64.0 * abs(gs)


# ------------------------------------------------------------------ runners (one per operator)
def run_logits(o, dev, c):
    cs = make(c)
    r = reference(c, 1.0)
    y, Wh, bh, lab, s4 = _dev(cs, dev)
    out = o.head_logits(y, Wh, bh, s4)
    path = o.last_path()
    N, H, W = cs.lab.shape
    ref = r.z.reshape(N, H, W, cs.K).permute(0, 3, 1, 2)
    if cs.mode != "gauss":
        xc.assert_exact(out, ref, "logits", "f32", 64.0, r.Lk.reshape(N, H, W, cs.K).permute(0, 3, 1, 2),
                        "head_logits")
    else:
        # C + 1 fp32 operations per logit: (C + 1) 2^-24 <= 2^-18 of the magnitude sum; factor 2
        bound = 2.0 ** -17 * r.Lk.reshape(N, H, W, cs.K).permute(0, 3, 1, 2)
        check_bound(out, ref, bound, "logits", "head_logits")
    return path, None


def run_fwd(o, dev, c):
    cs = make(c)
    r = reference(c, 1.0)
    y, Wh, bh, lab, s4 = _dev(cs, dev)
    out3 = o.head_ce_fwd(y, Wh, bh, lab, cs.ign, s4)
    path = o.last_path()
    exact = cs.mode == "sat"
    if exact:
        sat_precondition(cs, r)
    nb = min(-(-cs.P // 256), 2048)
    check_hits(cs, r, out3, cs.mode != "gauss")
    check_loss(cs, r, out3, exact, None if exact else bounds(cs, r, nb, False), "head_ce_fwd")
    # the grid is fixed by the binding (min(ceil(P / 256), 2048) workgroups of 256 pixels)
    return path, (cs.P, 256 * 2048)


def _check_rows_exact(cs, r, gs, dW, db, part, fam):
    qA, qW, q1, q2 = _q(cs, gs)
    aW = r.d.abs().t() @ r.A.abs()
    xc.assert_exact(dW, r.dW, "dWh", "rows", qW, aW, fam)
    xc.assert_exact(db, r.db, "dbh", "rows", abs(gs), r.d.abs().sum(0), fam)
    if part is not None:
        G, C = cs.G, cs.C
        rows = part.double().reshape(G, -1, 2, C).sum(1).cpu()
        t1, t2 = r.dyh.reshape(G, -1, C), (r.dyh * r.xh).reshape(G, -1, C)
        xc.assert_exact(rows[:, 0], t1.sum(1), "BN rows sum dyh", "rows", q1, t1.abs().sum(1), fam)
        xc.assert_exact(rows[:, 1], t2.sum(1), "BN rows sum dyh*xhat", "rows", q2, t2.abs().sum(1), fam)


def _check_rows_bound(cs, r, b, dW, db, part, fam, stored):
    # (stored: dW / db come back as one fp32 value rounded from the fp64 row sum)
    st = 2.0 ** -24 if stored else 0.0
    check_bound(dW, r.dW, b.dW + st * r.dW.abs(), "dWh", fam + ".dW")
    check_bound(db, r.db, b.db + st * r.db.abs(), "dbh", fam + ".db")
    if part is not None:
        G, C = cs.G, cs.C
        rows = part.double().reshape(G, -1, 2, C).sum(1).cpu()
        check_bound(rows[:, 0], r.dyh.reshape(G, -1, C).sum(1), b.p1, "BN rows sum dyh", fam + ".bn")
        check_bound(rows[:, 1], (r.dyh * r.xh).reshape(G, -1, C).sum(1), b.p2, "BN rows sum dyh*xhat", fam + ".bn")


def run_bwd(o, dev, c):
    """head_ce_bwd: store = plain / deferred one-pass; store=0: the stats pass"""
    cs = make(c)
    store = bool(c.get("store", 1))
    r1 = reference(c, 1.0)
    gs = _gscale(cs) / max(r1.count, 1)
    r = reference(c, gs)
    y, Wh, bh, lab, s4 = _dev(cs, dev)
    gsc = torch.tensor([_gscale(cs)], device=dev)
    dA, dW, db, part = o.head_ce_bwd(y, Wh, bh, lab, _out3(r, dev), gsc, cs.ign, None, None, s4, store)
    path = o.last_path()
    if cs.defer:
        rows = part.shape[0]
    elif dev == "cuda":   # (the same grid with and without the deferred BatchNorm: head_ce_bwd_blocks)
        rows = o.head_ce_bwd(y, Wh, bh, lab, _out3(r, dev), gsc, cs.ign, None, None,
                             xc.bn_stats4(cs.C, 1).to(dev), False)[3].shape[0]
    else:
        rows = 1
    fam = "head_ce_bwd"
    if not store:
        assert dA.numel() == 0
    if cs.mode == "sat":
        sat_precondition(cs, r)
        if store:
            xc.assert_exact(dA.reshape(-1, cs.C), r.dA, "dA", q=_q(cs, gs)[0], family=fam)
        _check_rows_exact(cs, r, gs, dW, db, part if cs.defer else None, fam)
    else:
        b = bounds(cs, r, rows, True)
        if store:
            check_bound(dA.reshape(-1, cs.C), r.dA, b.dA, "dA", fam + ".dA")
            # (for the docs: the share of the fp32 term eps S alone, beyond the bf16 store)
            g64 = dA.detach().double().cpu().reshape(-1, cs.C)
            over = ((g64 - r.dA).abs() - 2.0 ** -8 * r.dA.abs()).clamp_min(0) / (r.eps[:, None] * r.S).clamp_min(1e-300)
            RATIO[fam + ".dA.eps"] = max(RATIO.get(fam + ".dA.eps", 0.0), float(over.max()))
        _check_rows_bound(cs, r, b, dW, db, part if cs.defer else None, fam, True)
    return path, rows


def run_fwd_stats(o, dev, c):
    cs = make(c)
    r = reference(c, 1.0)
    y, Wh, bh, lab, s4 = _dev(cs, dev)
    out3, wrows, brows = o.head_ce_fwd_stats(y, Wh, bh, lab, cs.ign, s4, cs.G if cs.G > 1 else 0)
    path = o.last_path()
    rows = brows.shape[0]
    assert rows % cs.G == 0 and wrows.shape[0] == (rows if dev == "cuda" else 1)
    ws = wrows.double().sum(0).cpu()
    dW, db = ws[:cs.K * cs.C].reshape(cs.K, cs.C), ws[cs.K * cs.C:]
    fam = "head_ce_fwd_stats"
    exact = cs.mode == "sat"
    check_hits(cs, r, out3, cs.mode != "gauss")
    if exact:
        sat_precondition(cs, r)
        check_loss(cs, r, out3, True)
        _check_rows_exact(cs, r, 1.0, dW, db, brows, fam)
    else:
        b = bounds(cs, r, rows, False)
        check_loss(cs, r, out3, False, b, fam)
        _check_rows_bound(cs, r, b, dW, db, brows, fam, False)
    return path, rows


def run_bn_bwd(o, dev, c):
    """head_ce_bn_bwd: dY, dgamma, dbeta.  Without groups: bit-equal to head_ce_bwd storing dA
    followed by bn_backward on the same partial rows; in every case dY against the fp64
    formula k (dyh - m1 - xhat m2)."""
    cs = make(c)
    G, C = cs.G, cs.C
    r1 = reference(c, 1.0)
    gs = (1.0 if G > 1 else _gscale(cs)) / max(r1.count, 1)
    r = reference(c, gs)
    y, Wh, bh, lab, s4 = _dev(cs, dev)
    gamma = cs.gamma.to(dev)
    o3 = _out3(r, dev)
    if G > 1:   # the training path: unit-scale rows of the fused forward, scaled on the device
        _, _, part = o.head_ce_fwd_stats(y, Wh, bh, lab, cs.ign, s4, G)
        scale = o.head_grad_scale(o3, None)
        dY, dg, dbt = o.head_ce_bn_bwd(y, Wh, bh, lab, o3, None, cs.ign, s4, part, gamma, None, None, scale, G)
        path = o.last_path()
    else:
        gsc = torch.tensor([_gscale(cs)], device=dev)
        dA, _, _, part = o.head_ce_bwd(y, Wh, bh, lab, o3, gsc, cs.ign, None, None, s4, True)
        dY, dg, dbt = o.head_ce_bn_bwd(y, Wh, bh, lab, o3, gsc, cs.ign, s4, part, gamma)
        path = o.last_path()
        comp = o.bn_backward(dA, None, y, s4, gamma, None, None, None, part)
        for u, v, name in zip((dY, dg, dbt), comp, ("dY", "dgamma", "dbeta")):
            assert torch.equal(u, v), f"{name}: differs from head_ce_bwd + bn_backward"
    rows = part.shape[0]
    fam = "head_ce_bn_bwd"
    cnt = cs.P // G
    s = cs.s4.double().reshape(G, 4, C)
    k = (cs.gamma.double() * s[:, 1])[:, None, :]                              # [G][1][C]
    dyh, xh = r.dyh.reshape(G, -1, C), r.xh.reshape(G, -1, C)
    m1 = dyh.sum(1, keepdim=True) / cnt
    m2 = (dyh * xh).sum(1, keepdim=True) / cnt
    ref = k * (dyh - m1 - xh * m2)
    M1 = dyh.abs().sum(1, keepdim=True) / cnt
    M2 = (dyh * xh).abs().sum(1, keepdim=True) / cnt
    S = k.abs() * (dyh.abs() + M1 + xh.abs() * M2)
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * S
    gsum = (dyh * xh).sum((0, 1))
    bsum = dyh.sum((0, 1))
    gb = 2.0 ** -22 * (dyh * xh).abs().sum((0, 1))
    bb = 2.0 ** -22 * dyh.abs().sum((0, 1))
    if cs.mode == "sat":
        sat_precondition(cs, r)
    else:
        b = bounds(cs, r, rows, G == 1)
        e = b.edyh.reshape(G, -1, C)
        if G > 1:     # the apply pass always forms dyh from the bf16-rounded dA
            e = e + 2.0 ** -8 * dyh.abs()
        bound = bound + k.abs() * (e + b.p1[:, None, :] / cnt + xh.abs() * b.p2[:, None, :] / cnt)
        gb, bb = gb + b.p2.sum(0), bb + b.p1.sum(0)
    check_bound(dY.reshape(G, -1, C), ref, bound, "dY", fam + ".dY")
    check_bound(dg, gsum, gb, "dgamma", fam + ".dgamma")
    check_bound(dbt, bsum, bb, "dbeta", fam + ".dbeta")
    return path, rows


RUNNERS = {"logits": run_logits, "fwd": run_fwd, "bwd": run_bwd, "fwd_stats": run_fwd_stats,
           "bn_bwd": run_bn_bwd}


def loops(op, c, info):
    """does the case make its kernel's persistent loop iterate, judged from the row count the
    operator returned (GPU only)?  Returns (fact, requirement) for the assertion message."""
    P, C, G = c["N"] * c["H"] * c["W"], c["C"], max(c.get("groups", 0), 1)
    if op == "fwd":                            # grid-stride loop over 2 048 x 256 pixels
        return info[0], info[1]
    rows = info
    if C == 32:
        # waves = 4 per workgroup; a second trip of the D-deep step loop needs more than D steps
        # per wave.  The apply kernel returns no rows: the stats pass's count, and never more
        # than the 8 workgroups of 256 threads a CU can hold
        depth = 4 if op == "bn_bwd" else 3
        steps = -(-(P // G) // 16)
        need = depth * 4 * (rows // G)
        if op == "bn_bwd" and G == 1:
            need = max(need, depth * 4 * 8 * 8)
        return steps, need
    ppb = 256 // (C // 8)
    if op == "bn_bwd":                         # the apply kernel: 4 096 workgroups x 4 pixels per lane
        return P, 4096 * 4 * ppb
    return P, 2 * rows * ppb
