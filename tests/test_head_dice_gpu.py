"""Soft-Dice term through ``head_dice_fwd``, ``head_dice_coefs``, ``head_dice_bwd`` and
``head_dice_bn_bwd`` against an fp64 autograd reference of ``L = L_CE + lambda dice`` under the
bounds of ``head_cases.bounds`` (docs/TESTING.md, "Soft-Dice term").  ``num_cus()`` is pinned to 8;
P0 runs the tail lanes, at PLOOP every persistent loop takes a second trip.
"""
import pytest
import torch

import exact_cases as xc
import head_cases as hc

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAM, EPS, GSC = 0.5, 1.0, 0.75
P0, PLOOP = 16 * 37 + 5, 16 * 800 + 5


@pytest.fixture(scope="module")
def ops():
    o = xc.ops()
    if DEV != "cuda":
        yield o
        return
    try:
        o.set_cu_reserve(int(o.set_cu_reserve(0)) - 8)
        assert int(o.set_cu_reserve(-1)) == 8
        yield o
    finally:
        o.set_cu_reserve(0)


def inputs(C, K, defer, weights, P=P0, ignored=0.1):
    cs = hc.make(dict(mode="gauss", N=1, H=1, W=P, C=C, K=K, defer=int(defer), spread=0.3))
    g = torch.Generator().manual_seed(11)
    lab = cs.lab.reshape(-1).clone()
    lab[lab == K - 1] = 0                                             # the last class is absent
    lab[torch.rand(P, generator=g) < ignored] = cs.ign
    w = (torch.rand(K, generator=g) + 0.5) if weights else None
    return cs, lab, w


def reference(cs, lab, w):      # fp64, from the bf16-rounded activation and the fp32 weights
    r = hc.Ref()
    K, W = cs.K, cs.Wh.double()
    r.A = hc._act(cs)
    z = (r.A @ W.t() + cs.bh.double()).requires_grad_()
    r.L = (r.A.abs() @ W.abs().t() + cs.bh.double().abs()).max(1).values
    r.eps = 2.0 ** -15 * (1 + r.L)
    r.valid, r.am = lab != cs.ign, hc._first_max(z.detach())
    top = z.detach().topk(2, dim=1).values
    r.gap, r.hit = top[:, 0] - top[:, 1], r.am == lab
    r.hits, r.count = int(r.hit.sum()), int(r.valid.sum())
    v = r.valid.double()[:, None]
    hot = torch.nn.functional.one_hot(torch.where(r.valid, lab, torch.zeros_like(lab)), K).double() * v
    pw = v[:, 0] if w is None else (hot @ w.double())
    r.lse = torch.logsumexp(z, 1).detach()
    ce_px = -(torch.log_softmax(z, 1) * hot).sum(1) * pw
    r.pw, r.wsum = pw, float(pw.sum())                    # (the weight sum: out3[2], the CE's divisor)
    r.ce = ce_px.sum() / max(r.wsum, 1e-300)
    p = torch.softmax(z, 1) * v
    r.Ic, r.Sc, r.Yc = (p * hot).sum(0), p.sum(0), hot.sum(0)
    r.dice = (1 - ((2 * r.Ic + EPS) / (r.Sc + r.Yc + EPS)).mean()) if r.count else 0.0 * r.ce
    r.loss = r.ce + LAM * r.dice
    r.d, = torch.autograd.grad(GSC * r.loss, z)
    p, r.Ic, r.Sc, r.loss_px = p.detach(), r.Ic.detach(), r.Sc.detach(), ce_px.detach()
    r.ce, r.dice, r.loss = r.ce.detach(), r.dice.detach(), r.loss.detach()
    Dn = r.Sc + r.Yc + EPS
    g = (LAM * (2 * r.Ic + EPS) / (K * Dn ** 2) + hot * (2 * LAM / (K * Dn)))       # |B| + |A| [y = c]
    r.Dce = (p + hot) * pw[:, None] * GSC / max(r.wsum, 1e-300)
    r.Dd = p * (g + (p * g).sum(1, keepdim=True)) * GSC
    return r


def grads(cs, r, rows_fwd):
    W = cs.Wh.double()
    et = float(r.eps.max()) + hc._n_wg(cs, rows_fwd) * 2.0 ** -24 + 2.0 ** -23
    r.D = r.Dce + (1 + 2 * et / r.eps[:, None]) * r.Dd
    r.dA, r.S, r.dW, r.db = r.d @ W, r.D @ W.abs(), r.d.t() @ r.A, r.d.sum(0)
    if cs.defer:
        y = cs.y.double().reshape(-1, cs.C)
        r.mask = (y * hc._rows(cs, 2) + hc._rows(cs, 3)) > 0
        r.dyh = torch.where(r.mask, r.dA, torch.zeros_like(r.dA))
        r.xh = (y - hc._rows(cs, 0)) * hc._rows(cs, 1)
    return r


def check_dy(cs, r, b, dY, dg, dbt, fam):      # the dY bound of head_cases.run_bn_bwd, one group
    C, cnt = cs.C, cs.P
    k = (cs.gamma.double() * cs.s4.double().reshape(4, C)[1])[None, :]
    m1, m2 = r.dyh.sum(0, keepdim=True) / cnt, (r.dyh * r.xh).sum(0, keepdim=True) / cnt
    ref = k * (r.dyh - m1 - r.xh * m2)
    S = k.abs() * (r.dyh.abs() + r.dyh.abs().sum(0, keepdim=True) / cnt
                   + r.xh.abs() * (r.dyh * r.xh).abs().sum(0, keepdim=True) / cnt)
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * S + k.abs() * (b.edyh + b.p1 / cnt + r.xh.abs() * b.p2 / cnt)
    hc.check_bound(dY.reshape(-1, C), ref, bound, "dY", fam + ".dY")
    hc.check_bound(dg, (r.dyh * r.xh).sum(0), 2.0 ** -22 * (r.dyh * r.xh).abs().sum(0) + b.p2[0], "dgamma", fam + ".dgamma")
    hc.check_bound(dbt, r.dyh.sum(0), 2.0 ** -22 * r.dyh.abs().sum(0) + b.p1[0], "dbeta", fam + ".dbeta")


def run(o, cs, lab, w, tab_arg=True):
    t = lambda x: None if x is None else x.to(DEV)
    y, Wh, bh, s4, L, wd = t(cs.y), t(cs.Wh), t(cs.bh), t(cs.s4), t(lab.reshape(cs.lab.shape)), t(w)
    gsc = torch.tensor([GSC], device=DEV)
    out, paths = {}, []
    out["lrows"], out["drows"] = o.head_dice_fwd(y, Wh, bh, L, cs.ign, s4, wd)
    paths.append(o.last_path())
    out["out3"], out["tab"] = o.head_dice_coefs(out["lrows"], out["drows"], cs.K, LAM, EPS)
    tab = out["tab"] if tab_arg else None
    out["dA"], out["dW"], out["db"], out["part"] = o.head_dice_bwd(y, Wh, bh, L, out["out3"], gsc, cs.ign, None, None,
                                                                 s4, True, wd, tab)
    paths.append(o.last_path())
    if cs.defer:
        _, out["dW2"], out["db2"], out["part2"] = o.head_dice_bwd(y, Wh, bh, L, out["out3"], gsc, cs.ign, None, None,
                                                                s4, False, wd, tab)
        paths.append(o.last_path())
        out["dY"], out["dg"], out["dbt"] = o.head_dice_bn_bwd(y, Wh, bh, L, out["out3"], gsc, cs.ign, s4, out["part2"],
                                                            t(cs.gamma), None, None, None, 0, wd, tab)
        paths.append(o.last_path())
    return out, paths


CASES = [(C, K, d, wt, P0) for C, K in ((32, 6), (32, 16), (8, 2), (64, 5)) for d in (0, 1) for wt in (0, 1)]
CASES += [(32, 6, 1, 1, PLOOP), (64, 5, 1, 0, PLOOP)]          # every persistent loop takes a second trip


@pytest.mark.parametrize("C,K,defer,weights,P", CASES)
def test_dice(ops, C, K, defer, weights, P):
    cs, lab, w = inputs(C, K, defer, weights, P)
    assert int((lab == K - 1).sum()) == 0 and 0.05 < float((lab == cs.ign).double().mean()) < 0.15
    out, paths = run(ops, cs, lab, w)
    if DEV == "cuda":
        fam, dfr = ("head32" if C == 32 else "split"), (":defer" if defer else "")
        want = [f"head_dice_fwd:{fam}{dfr}", f"head_ce_bwd:{fam}{dfr}:dice"]
        want += [f"head_ce_bwd:{fam}:defer:stats:dice", f"head_ce_bn_bwd:{fam}:dice"] if defer else []
        assert paths == want, paths
    r = reference(cs, lab, w)
    rows_fwd, rows = out["drows"].shape[0], out["part"].shape[0] if defer else out["drows"].shape[0]
    acc = hc._n_wg(cs, rows_fwd) * 2.0 ** -24
    isy = out["drows"].double().sum(0).cpu()
    assert torch.equal(isy[2, :K], r.Yc) and float(isy[:, K:].abs().max() if K < 16 else 0.0) == 0.0
    hc.check_bound(isy[0, :K], r.Ic, acc * r.Ic, "I", "dice.I")
    hc.check_bound(isy[1, :K], r.Sc, acc * r.Sc, "S", "dice.S")
    o3, tab = out["out3"].double().cpu(), out["tab"].double().cpu()
    assert abs(float(o3[2]) - r.wsum) <= 2.0 ** -22 * r.wsum
    hc.check_hits(cs, r, o3 if w is None else torch.tensor([0.0, float(o3[1]), r.count]), False)
    bce = ((2.0 ** -16 * (1 + r.L) + 2.0 ** -22 * r.lse.abs()) * r.pw).sum() + acc * r.loss_px.sum()
    bce = float(bce) / max(r.wsum, 1e-300) + 2.0 ** -23 * float(r.ce)
    Dn = r.Sc + r.Yc + EPS
    bdice = float(((2 * r.Ic + (2 * r.Ic + EPS) * r.Sc / Dn) / Dn).mean()) * acc + 2.0 ** -23
    hc.check_bound(tab[33:34], r.ce.reshape(1), torch.tensor([bce]), "ce", "dice.ce")
    hc.check_bound(tab[32:33], r.dice.reshape(1), torch.tensor([bdice]), "dice", "dice.dice")
    hc.check_bound(o3[0:1], r.loss.reshape(1), torch.tensor([bce + LAM * bdice + 2.0 ** -23 * float(r.loss)]),
                   "L", "dice.L")
    assert float(tab[34:].abs().max()) == 0.0 and float(tab[K:16].abs().max() if K < 16 else 0.0) == 0.0
    grads(cs, r, rows_fwd)
    b = hc.bounds(cs, r, rows, True)
    hc.check_bound(out["dA"].reshape(-1, C), r.dA, b.dA, "dA", "dice.dA")
    hc._check_rows_bound(cs, r, b, out["dW"], out["db"], out["part"] if defer else None, "dice", True)
    if defer:
        hc._check_rows_bound(cs, r, b, out["dW2"], out["db2"], out["part2"], "dice.stats", True)
        check_dy(cs, r, b, out["dY"], out["dg"], out["dbt"], "dice")


@pytest.mark.parametrize("C,K", [(32, 6), (64, 5)])
def test_every_pixel_ignored(ops, C, K):
    cs, lab, w = inputs(C, K, 1, 1, ignored=2.0)
    out, _ = run(ops, cs, lab, w)
    for name, v in out.items():
        assert v.numel() and int((v != 0).sum()) == 0 and bool(torch.isfinite(v.float()).all()), name


@pytest.mark.parametrize("C,K", [(32, 6), (64, 5)])
def test_none_is_omitted_and_deterministic(ops, C, K):
    cs, lab, w = inputs(C, K, 1, 1)
    t = lambda x: x.to(DEV)
    y, Wh, bh, s4, L, wd, gsc = t(cs.y), t(cs.Wh), t(cs.bh), t(cs.s4), t(lab.reshape(cs.lab.shape)), t(w), torch.tensor([GSC], device=DEV)
    none, _ = run(ops, cs, lab, w, tab_arg=False)
    o3 = none["out3"]
    om = ops.head_ce_bwd(y, Wh, bh, L, o3, gsc, cs.ign, None, None, s4, False, wd)
    if DEV == "cuda":
        assert ops.last_path() == f"head_ce_bwd:{'head32' if C == 32 else 'split'}:defer:stats"
    oy = ops.head_ce_bn_bwd(y, Wh, bh, L, o3, gsc, cs.ign, s4, om[3], t(cs.gamma), None, None, None, 0, wd)
    for a, b_ in zip(list(om[1:]) + list(oy), [none[k] for k in ("dW2", "db2", "part2", "dY", "dg", "dbt")]):
        assert torch.equal(a, b_)
    one, _ = run(ops, cs, lab, w)
    two, _ = run(ops, cs, lab, w)
    assert float(one["dA"].float().sub(none["dA"].float()).abs().max()) > 0      # (the term is there)
    for name in one:
        assert torch.equal(one[name], two[name]), f"{name}: two runs differ"
