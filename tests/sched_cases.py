"""Cases for the scheduled optimizer step ``adam_step_sched`` (``csrc/optim.hip``, CPU twin in
``csrc/cpu_ref.cpp``): the gradient norm, the clip coefficient, the learning-rate schedule and
the clipped / decoupled update.  Written once and run on both kernel sets by
``test_sched_gpu.py`` and its ``test_sched_cpu.py`` mirror, as ``update_cases.py`` is; the Adam
helpers (``adam_ref``, ``adam_grad``, ``ulp32``, ``record``, ``assert_bits``) come from there.

Norm.  Integer-valued gradients ``k / 8``, ``|k| <= 8``: every square and every partial sum is
exact in fp64 whatever the order, so ``scal[4]`` must be ``float32(sqrt(exact sum))`` and
``scal[5]`` the fp32 cast of ``max_norm / (norm + 1e-6)`` (or 1.0) bit for bit.  General
gradients (``adam_grad``) are held to one fp32 ulp of ``sqrt(fsum(g^2))``.

Update.  Each step on its own, ``run_adam``'s method: the kernel's fp32 ``p, m, v`` before the
call and the device's own ``scal`` go into an fp64 evaluation of the documented expression
(``sched_ref``: ``adam_ref``'s bounds with one half-ulp term for ``g coef`` and one for
``p (1 - decay)``; docs/TESTING.md derives them).  With ``coef = 1`` and coupled decay the
results must be ``adam_step_dev``'s bit for bit.
"""
import math

import torch

from update_cases import (ADAM, SENT, U, _gen, adam_grad, adam_ref, assert_bits, f32, ops,  # noqa: F401
                          record, ulp32)

KINDS = ("constant", "poly", "cosine")
SQ_TRIP = 1024 * 256 * 4      # elements per trip of the norm kernel's capped grid (float4 loop)
SQ_BIG = 2 * SQ_TRIP + 3 * 1024 + 3
NORM_SIZES = [1, 3, 4, 1027, 10_007, SQ_BIG]


def blocks(n):
    from ddlpc.ops.adam import grad_sqnorm_blocks
    return grad_sqnorm_blocks(n)


def sched_call(o, p, g, m, v, scal, partial, wd=0.0, decoupled=False, max_norm=0.0, kind="constant",
               warmup=0, total=0, lr_min=0.0, power=0.9, lr=ADAM["lr"]):
    o.adam_step_sched(p, g, m, v, scal, partial, lr, ADAM["b1"], ADAM["b2"], ADAM["eps"], wd, decoupled,
                      max_norm, KINDS.index(kind), warmup, total, lr_min, power)


def state(dev, n, seed=21, offset=0):
    """p, g, m, v as views at `offset` floats into sentinel-filled buffers, scal[8], partial"""
    pad = 67

    def buf(init):
        big = torch.full((offset + n + pad,), SENT)
        big[offset:offset + n] = init
        big = big.to(dev)
        return big, big[offset:offset + n]
    bufs = [buf(torch.randn(n, generator=_gen(seed))), buf(torch.zeros(n)), buf(torch.zeros(n)),
            buf(torch.zeros(n))]
    scal = torch.zeros(8, device=dev)
    partial = torch.zeros(blocks(n), dtype=torch.float64, device=dev)
    return bufs, scal, partial


def untouched(bufs, offset, n):
    for name, (big, _) in zip("pgmv", bufs):
        b = big.cpu()
        assert bool((b[:offset] == SENT).all()) and bool((b[offset + n:] == SENT).all()), (
            f"{name}: written outside the view")


# ------------------------------------------------------------------ norm
def int_grad(n, seed):
    k = torch.randint(-8, 9, (n,), generator=_gen(seed))
    k[0] = 8                                   # (never an all-zero gradient)
    return k


def run_norm_exact(o, dev, n, offset=0):
    k = int_grad(n, 70 + n % 97)
    gc = (k.double() / 8).float()
    assert torch.equal(gc.double() * 8, k.double())
    exact = int((k * k).sum()) / 64.0          # an integer below 2^53 times 2^-6: exact
    norm = math.sqrt(exact)
    if n == SQ_BIG:
        assert blocks(n) == 1024 and (n // 4) // (1024 * 256) == 2 and (n // 4) % (1024 * 256) == 3 * 256 \
            and n % 4 == 3 and n < 5_000_000
    for max_norm, clipped in ((0.5 * norm, True), (2.0 * norm + 1.0, False)):
        bufs, scal, partial = state(dev, n, offset=offset)
        (_, p), (_, g), (_, m), (_, v) = bufs
        g.copy_(gc)
        sched_call(o, p, g, m, v, scal, partial, max_norm=max_norm)
        sc = scal.cpu()
        want = torch.tensor([norm, 1.0 if not clipped else max_norm / (norm + 1e-6)], dtype=torch.float64).float()
        assert_bits(sc[4:6], want, f"norm / coef n={n} max_norm={max_norm}")
        assert (float(sc[5]) < 1.0) == clipped
        assert float(partial.cpu()[:blocks(n)].sum()) == exact, "the partials do not sum to the exact sum"
        assert torch.equal(g.cpu(), gc), "the gradient was written"
        untouched(bufs, offset, n)


def run_norm_general(o, dev, n, offset=0):
    gc = adam_grad(n, 1, 23)
    if n < 14:
        gc[0] = 0.37
    ref = math.sqrt(math.fsum((gc.double() ** 2).tolist()))
    got = []
    devs = [dev] if dev == "cpu" else [dev, "cpu"]
    for d in devs:
        bufs, scal, partial = state(d, n, offset=offset)
        (_, p), (_, g), (_, m), (_, v) = bufs
        g.copy_(gc)
        sched_call(o, p, g, m, v, scal, partial, max_norm=1.0)
        a, pa = scal.cpu().clone(), partial.cpu().clone()
        sched_call(o, p, g, m, v, scal, partial, max_norm=1.0)
        assert_bits(scal.cpu()[4:6], a[4:6], f"norm / coef of a second call n={n} on {d}")
        assert torch.equal(partial.cpu(), pa), "partials of a second call"
        norm = float(a[4])
        print(f"norm n={n} {d}: {norm!r} ref {ref!r} err/ulp {abs(norm - ref) / ulp32(ref):.3f}")
        assert abs(norm - ref) <= ulp32(ref), (d, n, norm, ref)
        got.append(norm)
        untouched(bufs, offset, n)
    if len(got) == 2:
        assert abs(got[0] - got[1]) <= ulp32(ref), ("gpu vs cpu kernels", got)


# ------------------------------------------------------------------ reduces to adam_step_dev
def run_reduces(o, dev, n, wd, steps=5, seed=21):
    bufs, scal, partial = state(dev, n, seed)
    ref, _, _ = state(dev, n, seed)
    (_, p), (_, g), (_, m), (_, v) = bufs
    (_, p2), (_, g2), (_, m2), (_, v2) = ref
    scal3 = torch.zeros(3, device=dev)
    for t in range(1, steps + 1):
        gc = adam_grad(n, t, seed)
        g.copy_(gc)
        g2.copy_(gc)
        sched_call(o, p, g, m, v, scal, partial, wd=wd, max_norm=1e30)
        o.adam_step_dev(p2, g2, m2, v2, scal3, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], wd)
        sc = scal.cpu()
        assert float(sc[5]) == 1.0 and float(sc[4]) > 0.0 and float(sc[6]) == 0.0
        assert_bits(sc[:3], scal3.cpu(), f"scal[0..2] at step {t}")
        for name, a, b in (("p", p, p2), ("m", m, m2), ("v", v, v2)):
            assert_bits(a, b, f"{name} at step {t} (n={n}, wd={wd})")


# ------------------------------------------------------------------ update, per element
def sched_ref(p0, m0, v0, g, b1, b2, eps, wd, ss, inv, coef, dec, decoupled):
    """adam_ref with the two additions of adam_sched_kernel, every scalar the fp32 value the
    kernel reads:

        gc = g coef                        Egc = u |gc|                              (0 for coef = 1)
        coupled:    gr = gc + wd p         Egr = Egc + u (|wd p| + |gr|)             (Egc without wd)
                    p0 = p                 Ep0 = 0
        decoupled:  gr = gc                Egr = Egc
                    p0 = p keep            Ep0 = u |p0|       keep = fl(1 - dec), formed in fp32
        ... m', v', q as adam_ref ...
        p' = p0 - q                        Ep  = Ep0 + Eq + u |p'|
    """
    one = torch.tensor(1.0, dtype=torch.float32)
    omb1 = float(one - torch.tensor(b1, dtype=torch.float32))
    omb2 = float(one - torch.tensor(b2, dtype=torch.float32))
    keep = float(one - torch.tensor(dec, dtype=torch.float32))
    p, m, v = p0.double(), m0.double(), v0.double()
    gc = g.double() * coef
    Egc = U * gc.abs() if coef != 1.0 else torch.zeros_like(gc)
    if decoupled:
        gr, Egr = gc, Egc
        pk = p * keep
        Epk = U * pk.abs()
    else:
        pk, Epk = p, torch.zeros_like(p)
        if wd != 0.0:
            gr = gc + wd * p
            Egr = Egc + U * ((wd * p).abs() + gr.abs())
        else:
            gr, Egr = gc, Egc
    mr = m + omb1 * (gr - m)
    Em = omb1 * Egr + 2 * U * omb1 * (gr - m).abs() + U * mr.abs()
    vr = b2 * v + omb2 * gr * gr
    Ev = 2 * omb2 * gr.abs() * Egr + U * (b2 * v + 2 * omb2 * gr * gr + vr)
    s = vr.sqrt()
    lo = s + (vr - Ev).clamp_min(0.0).sqrt()
    Es = torch.where(lo > 0, Ev / lo.clamp_min(1e-300), torch.zeros_like(Ev)) + U * s
    d = s * inv + eps
    Ed = inv * Es + U * s * inv + U * d
    num = ss * mr
    q = num / d
    dlo = d - Ed
    assert bool((dlo > 0).all()), "bad case: the denominator is not bounded away from zero"
    Eq = (ss * Em + U * num.abs() + q.abs() * Ed) / dlo + U * q.abs()
    pr = pk - q
    Ep = Epk + Eq + U * pr.abs()
    k = 1 + 2.0 ** -10
    return (mr, k * Em), (vr, k * Ev), (pr, k * Ep)


def check_sched_ref():
    """without clipping and with coupled decay the reference is update_cases.adam_ref, exactly"""
    n = 1027
    p0, m0, v0 = torch.randn(n, generator=_gen(1)), torch.randn(n, generator=_gen(2)) * 1e-2, \
        torch.rand(n, generator=_gen(3)) * 1e-3
    g = adam_grad(n, 2, 5)
    for wd in (0.0, f32(0.01)):
        a = adam_ref(p0, m0, v0, g, f32(0.9), f32(0.999), f32(1e-8), wd, f32(1e-3), f32(1.5))
        b = sched_ref(p0, m0, v0, g, f32(0.9), f32(0.999), f32(1e-8), wd, f32(1e-3), f32(1.5), 1.0, 0.0, False)
        for (x, ex), (y, ey) in zip(a, b):
            assert torch.equal(x, y) and torch.equal(ex, ey)


def run_update(o, dev, n, wd, clip, decoupled, offset=0, steps=5, seed=21):
    """`steps` scheduled steps (poly, warm-up 2 of 10), each checked on its own against sched_ref"""
    b1, b2, eps = ADAM["b1"], ADAM["b2"], ADAM["eps"]
    bufs, scal, partial = state(dev, n, seed, offset)
    (_, p), (_, g), (_, m), (_, v) = bufs
    max_norm = 0.05 * math.sqrt(n) if clip else 0.0     # (adam_grad's norm is about 0.19 sqrt(n))
    fam = "adam_step_sched" + (" clip" if clip else "") + (" decoupled" if decoupled else "") + (" wd" if wd else "")
    nclipped = 0
    for t in range(1, steps + 1):
        gc = adam_grad(n, t, seed)
        g.copy_(gc)
        p0, m0, v0 = p.cpu().clone(), m.cpu().clone(), v.cpu().clone()
        sched_call(o, p, g, m, v, scal, partial, wd=wd, decoupled=decoupled, max_norm=max_norm, kind="poly",
                   warmup=2, total=10, lr_min=1e-5)
        sc = [float(x) for x in scal.cpu()]
        assert sc[0] == float(t) and sc[7] == 0.0
        if clip:
            # (n = 1: adam_grad's element 0 is zero at every step — norm 0, coef 1)
            assert 0.0 < sc[5] <= 1.0 and (sc[4] > 0.0 or not bool(gc.any()))
            nclipped += sc[5] < 1.0
        else:
            assert sc[5] == 1.0 and sc[4] == 0.0
        assert (sc[6] > 0.0) == (decoupled and wd != 0.0)
        (mr, Em), (vr, Ev), (pr, Ep) = sched_ref(p0, m0, v0, gc, f32(b1), f32(b2), f32(eps), f32(wd), sc[1],
                                                 sc[2], sc[5], sc[6], decoupled)
        record(fam + " m", m.cpu(), mr, Em)
        record(fam + " v", v.cpu(), vr, Ev)
        record(fam + " p", p.cpu(), pr, Ep)
        assert torch.equal(g.cpu(), gc), "the gradient was written"
    assert not clip or n < 1027 or nclipped == steps, "bad case: max_norm does not clip"
    untouched(bufs, offset, n)


# ------------------------------------------------------------------ schedule
SCHED = dict(W=5, T=30, lr_min=1e-5, steps=40)


def run_schedule(o, dev, kind, power):
    from ddlpc.ops.adam import schedule_lr
    lr, b1, b2 = ADAM["lr"], ADAM["b1"], ADAM["b2"]
    W, T, lr_min = SCHED["W"], SCHED["T"], SCHED["lr_min"]
    bufs, scal, partial = state(dev, 3)
    (_, p), (_, g), (_, m), (_, v) = bufs
    g.copy_(torch.tensor([0.5, -0.25, 0.0]))
    exact = kind == "constant" or (kind == "poly" and power == 1.0)
    seen = []
    for t in range(1, SCHED["steps"] + 1):
        sched_call(o, p, g, m, v, scal, partial, kind=kind, warmup=W, total=T, lr_min=lr_min, power=power)
        sc = [float(x) for x in scal.cpu()]
        lr_t = schedule_lr(t, lr, kind, W, T, lr_min, power)
        assert sc[0] == float(t)
        if exact:
            assert sc[3] == f32(lr_t), (kind, power, t, sc[3], lr_t)
        for got, want, what in ((sc[3], lr_t, "lr_t"), (sc[1], lr_t / (1 - b1 ** t), "step_size"),
                                (sc[2], 1 / math.sqrt(1 - b2 ** t), "inv_sqrt_bc2")):
            assert abs(got - want) <= ulp32(want), (kind, power, t, what, got, want)
        if t > T and kind != "constant":
            assert sc[3] == f32(lr_min), (kind, t, sc[3])
        seen.append(lr_t)
    # the twin itself: warm-up ramps to lr at step W, the decay falls monotonically to lr_min
    assert seen[0] == lr * 1.0 / W and math.isclose(seen[W - 1], lr, rel_tol=1e-15) and seen[W] == lr_min + (lr - lr_min)
    if kind == "constant":
        assert all(x == seen[W] for x in seen[W:])
    else:
        assert all(a > b for a, b in zip(seen[W:T], seen[W + 1:T + 1])) and seen[T] == lr_min == seen[-1]


# ------------------------------------------------------------------ bindings
def run_empty(o, dev):
    e = [torch.zeros(0, device=dev) for _ in range(4)]
    scal = torch.zeros(8, device=dev)
    for max_norm in (0.0, 1.0):
        sched_call(o, *e, scal, torch.zeros(0, dtype=torch.float64, device=dev), max_norm=max_norm)
    sc = scal.cpu()
    assert float(sc[0]) == 2.0 and float(sc[5]) == 1.0 and float(sc[4]) == 0.0 and float(sc[3]) == f32(ADAM["lr"])


def binding_calls(o, dev):
    """name -> a call the GPU binding must refuse (TORCH_CHECK) before any launch"""
    n = 2048                                    # two partial sums
    f = lambda *s, dt=torch.float32, d=dev: torch.zeros(*s, dtype=dt, device=d)
    strided = lambda: f(2 * n)[::2]
    assert blocks(n) == 2

    def call(scal=None, partial=None, kind="constant", **kw):
        b = {k: (f(n) if kw.get(k) is None else kw[k]) for k in "pgmv"}
        sched_call(o, b["p"], b["g"], b["m"], b["v"], f(8) if scal is None else scal,
                   f(2, dt=torch.float64) if partial is None else partial, max_norm=1.0)
    out = {}
    for k in "pgmv":
        out[f"{k} strided"] = lambda k=k: call(**{k: strided()})
        out[f"{k} fp64"] = lambda k=k: call(**{k: f(n, dt=torch.float64)})
        out[f"{k} shorter"] = lambda k=k: call(**{k: f(n - 1)})
    for k in "gmv":
        out[f"{k} on the host"] = lambda k=k: call(**{k: f(n, d="cpu")})
    out.update({
        "scal short": lambda: call(scal=f(7)),
        "scal float[3]": lambda: call(scal=f(3)),
        "scal fp64": lambda: call(scal=f(8, dt=torch.float64)),
        "scal on the host": lambda: call(scal=f(8, d="cpu")),
        "partial fp32": lambda: call(partial=f(2)),
        "partial short": lambda: call(partial=f(1, dt=torch.float64)),
        "partial on the host": lambda: call(partial=f(2, dt=torch.float64, d="cpu")),
        "sched_kind 3": lambda: o.adam_step_sched(f(n), f(n), f(n), f(n), f(8), f(2, dt=torch.float64), 1e-3, 0.9,
                                                  0.999, 1e-8, 0.0, False, 0.0, 3, 0, 0, 0.0, 0.9),
    })
    return out


BINDING_NAMES = list(binding_calls(None, "cpu"))      # (the calls are built lazily: none runs here)
