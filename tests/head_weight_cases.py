"""Class-weighted cases for the 1x1 head / cross-entropy operators (``class_weight=``), written
once and run on both kernel sets: ``test_head_weighted_gpu.py`` (``csrc/head_ce.hip``) and its
``test_head_weighted_cpu.py`` mirror (``csrc/cpu_ref.cpp``).  docs/TESTING.md, "Head and
cross-entropy: class weights", has the derivation and the worst figures.

The weighted fp64 reference.  Every quantity derived from the softmax-CE gradient ``d`` is
linear in ``d`` per pixel, so the reference is ``head_cases.reference(c, 1.0)`` (cached there;
copied here, never mutated) with ``d, D, dA, S, dW, db, dyh`` scaled per pixel by
``s_p = w[label_p] * gs``, ``gs = gscale / sum_p w[label_p]`` (1 for the unit-scale forward), the
loss terms scaled by ``w[label_p]`` and ``count`` replaced by the weight sum.  Hits stay
unweighted.

Saturated cases: weights from {1/2, 1, 2}; ``drop_to_pow2`` ignores extra pixels until the weight
sum of the valid ones is a power of two, so ``gs``, ``gs * w`` and every output stay exact (the
quantum of ``head_cases._q`` halves, the magnitudes at most double: <= 4 x 1.88 M = 7.5 M quanta
against 2^24).  Gaussian cases: six arbitrary weights from 0.3 to 3, one exactly 0, the bounds of
``head_cases.bounds`` evaluated on the weighted reference plus one fp32 rounding (2^-24
relative) per weighted product.
"""
import copy
import math

import torch

import exact_cases as xc
import head_cases as hc

# shapes of test_head_exact_gpu.py (the persistent loops wrap at 8 CUs; see there)
S32 = dict(N=2, H=61, W=67, C=32)
S32A = dict(N=2, H=91, W=93, C=32)
S64 = dict(N=2, H=47, W=45, C=64)
S16 = dict(N=2, H=91, W=95, C=16)
S8 = dict(N=2, H=129, W=129, C=8)
G3 = dict(N=9, H=20, W=44, C=32, groups=3, defer=1)
G5 = dict(N=10, H=20, W=44, C=32, groups=5, defer=1)

GAUSS_W = [0.3, 0.0, 3.0, 0.7, 1.9, 1.0]     # six values from 0.3 to 3, one exactly 0


def sat_weights(K, seed=0):
    """weights from {1/2, 1, 2}: all three present for K >= 3"""
    return torch.tensor([[2.0, 0.5, 1.0][(k + seed) % 3] for k in range(K)])


def gauss_weights(K):
    return torch.tensor([GAUSS_W[k % 6] for k in range(K)])


# ------------------------------------------------------------------ the weighted case + reference
def drop_to_pow2(cs, r1, w):
    """mask of extra pixels to ignore so that the weight sum of the remaining valid pixels is a
    power of two (weights are multiples of 1/2), chosen by a seeded permutation"""
    lab = cs.lab.reshape(-1)
    wpx = torch.where(r1.valid, w.double()[lab.clamp(0, cs.K - 1)], torch.zeros(cs.P, dtype=torch.float64))
    total = float(wpx.sum())
    drop = torch.zeros(cs.P, dtype=torch.bool)
    if total <= 0:
        return drop
    deficit = total - 2.0 ** math.floor(math.log2(total))
    g = torch.Generator().manual_seed(cs.c.get("seed", 7) + 101)
    perm = torch.randperm(cs.P, generator=g)
    # a random prefix of the permutation (every class loses the same share), then single
    # pixels of the remaining tail that still fit
    wp = wpx[perm]
    n = int((wp.cumsum(0) <= deficit).sum())
    drop[perm[:n]] = True
    deficit -= float(wp[:n].sum())
    for i in perm[n:].tolist():
        if deficit == 0:
            break
        if 0 < float(wpx[i]) <= deficit:
            drop[i] = True
            deficit -= float(wpx[i])
    assert deficit == 0, f"bad case: cannot reach a power-of-two weight sum (left {deficit})"
    return drop


def wcase(c, w, gscale, pow2):
    """-> (case copy with the extra ignored pixels, weighted fp64 reference at
    gs = gscale / weight sum; gscale None: the unit-scale pass, gs = 1)"""
    cs0 = hc.make(c)
    r1 = hc.reference(c, 1.0)
    drop = drop_to_pow2(cs0, r1, w) if pow2 else torch.zeros(cs0.P, dtype=torch.bool)
    cs = copy.copy(cs0)
    lab0 = cs0.lab.reshape(-1)
    cs.lab = torch.where(drop, torch.full_like(lab0, cs0.ign), lab0).reshape(cs0.lab.shape).contiguous()
    r = copy.copy(r1)
    r.valid = r1.valid & ~drop
    r.npix = int(r.valid.sum())
    r.wpx = torch.where(r.valid, w.double()[lab0.clamp(0, cs.K - 1)], torch.zeros(cs.P, dtype=torch.float64))
    r.wsum = float(r.wpx.sum())
    r.count = r.wsum
    r.hit = r1.hit & ~drop
    r.hits = int(r.hit.sum())
    r.loss_px = r1.loss_px * r.wpx
    r.loss = float(r.loss_px.sum()) / r.wsum if r.wsum > 0 else 0.0
    r.gs = 1.0 if gscale is None else gscale / (r.wsum if r.wsum > 0 else 1.0)
    s = (r.wpx * r.gs)[:, None]
    r.d, r.D = r1.d * s, r1.D * s.abs()
    r.dA, r.S = r1.dA * s, r1.S * s.abs()
    r.dW, r.db = r.d.t() @ r.A, r.d.sum(0)
    if cs.defer:
        r.dyh = r1.dyh * s
    if pow2:
        assert r.wsum > 0 and math.log2(r.wsum) == round(math.log2(r.wsum)), f"bad case: weight sum {r.wsum}"
    return cs, r


def sat_precondition(cs, r):
    """head_cases.sat_precondition on the pixels (its shares are shares of the valid pixels)"""
    rp = copy.copy(r)
    rp.count = r.npix
    hc.sat_precondition(cs, rp)


def _dev(cs, w, dev):
    return hc._dev(cs, dev) + (w.float().to(dev),)


def _out3(r, dev):
    return torch.tensor([r.loss, float(r.hits), r.wsum], dtype=torch.float32, device=dev)


# ------------------------------------------------------------------ bounds
def wbounds(cs, r, rows, rounded, nprod):
    """head_cases.bounds on the weighted reference (its terms are linear in d, D, dA, S, dyh, so
    they carry the weights already), the loss terms weighted, plus ``nprod`` fp32 roundings of the
    per-pixel scale (2^-24 relative each: out3[2] stored as fp32, gs * w; the forward's
    (lse - z_y) * w): every d-derived quantity moves by at most nprod 2^-24 of its magnitude
    sum."""
    b = hc.bounds(cs, r, rows, rounded)
    u = nprod * 2.0 ** -24
    acc = hc._n_wg(cs, rows) * 2.0 ** -24
    b.dA = b.dA + u * r.S
    b.dW = b.dW + u * (r.d.abs().t() @ r.A.abs())
    b.db = b.db + u * r.d.abs().sum(0)
    b.loss = b.loss * r.wpx + u * r.loss_px.abs()
    b.loss_sum = b.loss.sum() + acc * r.loss_px.abs().sum()
    b.count = torch.tensor(acc * r.wsum, dtype=torch.float64)   # fp32 accumulation of the weights
    if cs.defer:
        G = cs.G
        m = r.mask.double()
        b.edyh = b.edyh + u * r.S * m
        b.p1 = b.p1 + u * (r.S * m).reshape(G, -1, cs.C).sum(1)
        b.p2 = b.p2 + u * (r.S * m * r.xh.abs()).reshape(G, -1, cs.C).sum(1)
    return b


def check_out3(cs, r, out3, exact, b, fam):
    """hits (unweighted; first maximum), the weight sum and the weighted mean loss"""
    got = out3.detach().double().cpu()
    cnt, hits = float(got[2]), float(got[1])
    if cs.mode != "gauss":
        assert hits == r.hits, f"hits {hits} != {r.hits} (first-maximum reference)"
    else:
        amb = r.valid & (r.gap < 2.0 ** -14 * (1 + r.L))
        assert int(amb.sum()) <= 0.001 * r.npix, f"bad case: {int(amb.sum())} ambiguous pixels"
        lo, hi = r.hits - int((amb & r.hit).sum()), r.hits + int((amb & ~r.hit).sum())
        assert lo <= hits <= hi, (lo, hits, hi)
    if exact:
        assert cnt == r.wsum, (cnt, r.wsum)
        # the exact sums divided in fp64 and rounded once: what ce_finalize computes
        assert r.loss_px.abs().sum() < xc.F32_EXACT * 64          # quantum 128 x 1/2
        q = r.loss_px / 64.0
        assert torch.equal(q, q.round())
        want = torch.tensor(r.loss_px.sum().item() / max(r.wsum, 1.0), dtype=torch.float64).float()
        assert float(out3[0]) == float(want), (float(out3[0]), float(want))
    else:
        hc.check_bound(got[2:3], torch.tensor([r.wsum], dtype=torch.float64), (b.count + 2.0 ** -24 * r.wsum).reshape(1),
                       "weight sum", fam + ".count")
        ref = torch.tensor([r.loss_px.sum().item()], dtype=torch.float64)
        # loss * (reference weight sum) against the weighted loss sum: the kernel divided by
        # ITS weight sum, so the weight sum's own error enters relative to the loss
        bound = b.loss_sum.reshape(1) + 2.0 ** -23 * ref.abs() + ref.abs() * (b.count / max(r.wsum, 1e-300) + 2.0 ** -24)
        hc.check_bound(got[0:1] * r.wsum, ref, bound, "loss sum", fam + ".loss")


# ------------------------------------------------------------------ runners (one per operator)
def run_fwd(o, dev, c, w):
    exact = c["mode"] == "sat"
    cs, r = wcase(c, w, None, exact)
    y, Wh, bh, lab, s4, cw = _dev(cs, w, dev)
    out3 = o.head_ce_fwd(y, Wh, bh, lab, cs.ign, s4, cw)
    path = o.last_path()
    if exact:
        sat_precondition(cs, r)
    nb = min(-(-cs.P // 256), 2048)
    check_out3(cs, r, out3, exact, None if exact else wbounds(cs, r, nb, False, 1), "w.head_ce_fwd")
    return path, (cs.P, 256 * 2048)


def _rows_exact(cs, r, dW, db, part, fam):
    hc._check_rows_exact(cs, r, r.gs * 0.5, dW, db, part, fam)      # (the quantum halves: w = 1/2)


def run_bwd(o, dev, c, w):
    exact = c["mode"] == "sat"
    store = bool(c.get("store", 1))
    cs0 = hc.make(c)
    cs, r = wcase(c, w, hc._gscale(cs0), exact)
    y, Wh, bh, lab, s4, cw = _dev(cs, w, dev)
    gsc = torch.tensor([hc._gscale(cs0)], device=dev)
    dA, dW, db, part = o.head_ce_bwd(y, Wh, bh, lab, _out3(r, dev), gsc, cs.ign, None, None, s4, store, cw)
    path = o.last_path()
    if cs.defer:
        rows = part.shape[0]
    elif dev == "cuda":     # (the same grid with and without the deferred BatchNorm)
        rows = o.head_ce_bwd(y, Wh, bh, lab, _out3(r, dev), gsc, cs.ign, None, None,
                             xc.bn_stats4(cs.C, 1).to(dev), False, cw)[3].shape[0]
    else:
        rows = 1
    fam = "w.head_ce_bwd"
    if not store:
        assert dA.numel() == 0
    if exact:
        sat_precondition(cs, r)
        if store:
            xc.assert_exact(dA.reshape(-1, cs.C), r.dA, "dA", q=hc._q(cs, r.gs * 0.5)[0], family=fam)
        _rows_exact(cs, r, dW, db, part if cs.defer else None, fam)
    else:
        b = wbounds(cs, r, rows, True, 2)
        if store:
            hc.check_bound(dA.reshape(-1, cs.C), r.dA, b.dA, "dA", fam + ".dA")
        hc._check_rows_bound(cs, r, b, dW, db, part if cs.defer else None, fam, True)
    return path, rows


def run_fwd_stats(o, dev, c, w):
    exact = c["mode"] == "sat"
    cs, r = wcase(c, w, None, exact)
    y, Wh, bh, lab, s4, cw = _dev(cs, w, dev)
    out3, wrows, brows = o.head_ce_fwd_stats(y, Wh, bh, lab, cs.ign, s4, cs.G if cs.G > 1 else 0, cw)
    path = o.last_path()
    rows = brows.shape[0]
    assert rows % cs.G == 0 and wrows.shape[0] == (rows if dev == "cuda" else 1)
    ws = wrows.double().sum(0).cpu()
    dW, db = ws[:cs.K * cs.C].reshape(cs.K, cs.C), ws[cs.K * cs.C:]
    fam = "w.head_ce_fwd_stats"
    if exact:
        sat_precondition(cs, r)
        check_out3(cs, r, out3, True, None, fam)
        _rows_exact(cs, r, dW, db, brows, fam)
    else:
        b = wbounds(cs, r, rows, False, 1)
        check_out3(cs, r, out3, False, b, fam)
        hc._check_rows_bound(cs, r, b, dW, db, brows, fam, False)
    return path, rows


def run_bn_bwd(o, dev, c, w):
    """head_ce_bn_bwd with weights, as head_cases.run_bn_bwd: without groups bit-equal to
    head_ce_bwd (same weights) storing dA followed by bn_backward; dY against the fp64 formula."""
    exact = c["mode"] == "sat"
    cs0 = hc.make(c)
    G, C = cs0.G, cs0.C
    cs, r = wcase(c, w, 1.0 if G > 1 else hc._gscale(cs0), exact)
    y, Wh, bh, lab, s4, cw = _dev(cs, w, dev)
    gamma = cs.gamma.to(dev)
    o3 = _out3(r, dev)
    if G > 1:
        _, _, part = o.head_ce_fwd_stats(y, Wh, bh, lab, cs.ign, s4, G, cw)
        scale = o.head_grad_scale(o3, None)
        dY, dg, dbt = o.head_ce_bn_bwd(y, Wh, bh, lab, o3, None, cs.ign, s4, part, gamma, None, None, scale, G, cw)
        path = o.last_path()
    else:
        gsc = torch.tensor([hc._gscale(cs0)], device=dev)
        dA, _, _, part = o.head_ce_bwd(y, Wh, bh, lab, o3, gsc, cs.ign, None, None, s4, True, cw)
        dY, dg, dbt = o.head_ce_bn_bwd(y, Wh, bh, lab, o3, gsc, cs.ign, s4, part, gamma, None, None, None, 0, cw)
        path = o.last_path()
        comp = o.bn_backward(dA, None, y, s4, gamma, None, None, None, part)
        for u, v, name in zip((dY, dg, dbt), comp, ("dY", "dgamma", "dbeta")):
            assert torch.equal(u, v), f"{name}: differs from head_ce_bwd + bn_backward"
    rows = part.shape[0]
    fam = "w.head_ce_bn_bwd"
    cnt = cs.P // G
    s = cs.s4.double().reshape(G, 4, C)
    k = (cs.gamma.double() * s[:, 1])[:, None, :]
    dyh, xh = r.dyh.reshape(G, -1, C), r.xh.reshape(G, -1, C)
    m1 = dyh.sum(1, keepdim=True) / cnt
    m2 = (dyh * xh).sum(1, keepdim=True) / cnt
    ref = k * (dyh - m1 - xh * m2)
    M1 = dyh.abs().sum(1, keepdim=True) / cnt
    M2 = (dyh * xh).abs().sum(1, keepdim=True) / cnt
    S = k.abs() * (dyh.abs() + M1 + xh.abs() * M2)
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * S
    gsum, bsum = (dyh * xh).sum((0, 1)), dyh.sum((0, 1))
    gb = 2.0 ** -22 * (dyh * xh).abs().sum((0, 1))
    bb = 2.0 ** -22 * dyh.abs().sum((0, 1))
    if exact:
        sat_precondition(cs, r)
    else:
        b = wbounds(cs, r, rows, G == 1, 2)
        e = b.edyh.reshape(G, -1, C)
        if G > 1:
            e = e + 2.0 ** -8 * dyh.abs()
        bound = bound + k.abs() * (e + b.p1[:, None, :] / cnt + xh.abs() * b.p2[:, None, :] / cnt)
        gb, bb = gb + b.p2.sum(0), bb + b.p1.sum(0)
    hc.check_bound(dY.reshape(G, -1, C), ref, bound, "dY", fam + ".dY")
    hc.check_bound(dg, gsum, gb, "dgamma", fam + ".dgamma")
    hc.check_bound(dbt, bsum, bb, "dbeta", fam + ".dbeta")
    return path, rows


RUNNERS = {"fwd": run_fwd, "bwd": run_bwd, "fwd_stats": run_fwd_stats, "bn_bwd": run_bn_bwd}


# ------------------------------------------------------------------ identities and edge runs
def all_ops(o, dev, cs, cw, mode, omit=False):
    """every weighted operator on one (deferred-BN) case -> dict of output tensors.  mode "kw":
    class_weight passed (None included); omit: the argument left out entirely.  The backward
    operators take the forward's own out3; the unit-scale rows are turned into gradients by
    head_wgrad_from_rows / pscale as the engine does."""
    y, Wh, bh, lab, s4 = hc._dev(cs, dev)
    gamma = cs.gamma.to(dev)
    kw = {} if omit else {"class_weight": cw}
    gsc = torch.tensor([0.75], device=dev)
    out = {}
    out["fwd.out3"] = o.head_ce_fwd(y, Wh, bh, lab, cs.ign, s4, **kw)
    o3, wrows, brows = o.head_ce_fwd_stats(y, Wh, bh, lab, cs.ign, s4, 0, **kw)
    out["fwd_stats.out3"] = o3
    scale = o.head_grad_scale(o3, gsc)
    out["fwd_stats.dW"], out["fwd_stats.db"] = o.head_wgrad_from_rows(wrows, scale, cs.K, cs.C)
    out["rows.w"], out["rows.bn"] = wrows, brows
    for store in (True, False):
        dA, dW, db, part = o.head_ce_bwd(y, Wh, bh, lab, o3, gsc, cs.ign, None, None, s4, store, **kw)
        t = "bwd" if store else "bwd_stats"
        out[t + ".dW"], out[t + ".db"], out[t + ".part"] = dW, db, part
        if store:
            out["bwd.dA"] = dA
    dAp = o.head_ce_bwd(y, Wh, bh, lab, o3, gsc, cs.ign, None, None, None, True, **kw)
    out["bwd_plain.dA"], out["bwd_plain.dW"], out["bwd_plain.db"] = dAp[0], dAp[1], dAp[2]
    r = o.head_ce_bn_bwd(y, Wh, bh, lab, o3, gsc, cs.ign, s4, out["bwd.part"], gamma, None, None, None, 0, **kw)
    out["bn_bwd.dY"], out["bn_bwd.dg"], out["bn_bwd.db"] = r
    r = o.head_ce_bn_bwd(y, Wh, bh, lab, o3, gsc, cs.ign, s4, brows, gamma, None, None, scale, 0, **kw)
    out["bn_bwd_ps.dY"], out["bn_bwd_ps.dg"], out["bn_bwd_ps.db"] = r
    return out


GRADS = ["fwd_stats.dW", "fwd_stats.db", "bwd.dW", "bwd.db", "bwd.part", "bwd.dA", "bwd_stats.dW",
         "bwd_stats.db", "bwd_stats.part", "bwd_plain.dA", "bwd_plain.dW", "bwd_plain.db",
         "bn_bwd.dY", "bn_bwd.dg", "bn_bwd.db", "bn_bwd_ps.dY", "bn_bwd_ps.dg", "bn_bwd_ps.db"]


def relabel(cs, lab):
    c2 = copy.copy(cs)
    c2.lab = lab.reshape(cs.lab.shape).contiguous()
    return c2
