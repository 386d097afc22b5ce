"""Exact cases for the other half of a training step: the lossy gradient codec (``codec_absmax``,
``codec_encode``, ``codec_decode_sum``), the flat Adam update (``adam_step``, ``adam_step_dev``),
the one-launch ``weight_pack`` and the input conversion ``to_nhwc_bf16``.  Written once and run on
both kernel sets: ``test_update_exact_gpu.py`` (the gfx950 kernels of ``csrc/misc.hip``) and its
``test_update_exact_cpu.py`` mirror (``csrc/cpu_ref.cpp``).

Codec.  The reference is the torch oracle ``ddlpc.parallel.codec`` run on the CPU; payloads are
compared by bit pattern (fp16 viewed as int16, so ``-0.0`` counts) and scales with ``torch.equal``.
One flat buffer holds segments at odd offsets (``seg_table``): one element, 257 elements, an empty
segment, one that ends off a multiple of 4, one of 2 * 65 536 + 17 elements (three trips of the
encode / decode grid-stride loops, nine of absmax) and gaps that belong to no segment.  Tie cases
make ``g / scale * L`` exact in fp32 with every second level a rounding tie.  A decode with weights
that are powers of two must equal the oracle's rank-order fp32 accumulation bit for bit (``w d`` is
exact, so an FMA cannot change it); with general weights it is held per element to an fp64
reference within ``world 2^-24 sum |w_r d_r|`` (one rounding per product, one per addition).

Adam.  Every step is compared on its own: the kernel's fp32 ``p, m, v`` before the call go into
an fp64 evaluation of the kernel's expression with the fp32-rounded scalars, and each of the three
results is bounded by the roundings of that expression (``adam_ref`` derives them), with the
rounding of ``gr = g + wd p`` propagated.  Contraction to FMAs only removes roundings, so the CPU
and the GPU kernels share the bounds.

``weight_pack`` and ``to_nhwc_bf16`` are permutations with one bf16 rounding: bit-exact against a
``permute(...).bfloat16()`` written out here, on values of which three quarters lie on or next to
a bf16 rounding tie.

``WORST`` collects the worst observed error / bound of the bounded quantities and ``TIES`` the tie
shares (records for docs/TESTING.md, not tolerances).
"""
import math

import torch

from exact_cases import ops  # noqa: F401

WORST = {}            # family -> worst |got - ref| / bound
TIES = {}             # case -> share of the elements on a rounding tie

CODECS = ("fp16_absmax", "int8_absmax")
SENT = -77.0          # fp32 / bf16 sentinel (exact in both)
QSENT = 55            # payload sentinel (fp16 55.0 / int8 55)
U = 2.0 ** -24        # unit roundoff of fp32


def codec_mods():
    from ddlpc.ops import codec_ops
    from ddlpc.parallel import codec as oracle
    return codec_ops, oracle


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    """the bit patterns of a tensor (on the CPU)"""
    t = t.detach().cpu().contiguous()
    view = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
    return t.view(view[t.dtype]) if t.dtype in view else t


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    bad = g != w
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first "
                                 f"{bad.nonzero()[:6].flatten().tolist()}")


def record(fam, got, ref, bound):
    """worst |got - ref| / bound of a bounded quantity, then the assertion"""
    g, ref, bound = got.detach().double().cpu(), ref.double(), bound.double()
    err = (g - ref).abs()
    err = torch.where(torch.isnan(err), torch.tensor(math.inf, dtype=torch.float64), err)
    ratio = torch.where(bound > 0, err / bound,
                        torch.where(err > 0, torch.tensor(math.inf, dtype=torch.float64),
                                    torch.tensor(0.0, dtype=torch.float64)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    bad = err > bound
    assert not bool(bad.any()), (f"{fam}: {int(bad.sum())} of {bad.numel()} outside the bound, first "
                                 f"{bad.nonzero()[:4].flatten().tolist()}, worst ratio {worst:.3f}")


def rounding_mix(shape, seed):
    """fp32 Gaussian values of which a quarter each lie exactly on a bf16 rounding tie (low half
    0x8000), just above it (0x8001: rounds up in magnitude) and just below (0x7fff: rounds down);
    the last quarter is left as drawn -> (values, share on a tie)"""
    g = _gen(seed)
    x = torch.randn(shape, generator=g).contiguous()
    kind = torch.randint(0, 4, shape, generator=g)
    low = torch.tensor([0x8000, 0x8001, 0x7fff, 0], dtype=torch.int32)[kind]
    b = x.view(torch.int32)
    b = torch.where(kind < 3, (b & -65536) | low, b)
    return b.view(torch.float32), float((kind == 0).double().mean())


# ------------------------------------------------------------------ codec: the segment table
BIG = 2 * 65536 + 17
ENC_TRIP = 256 * 256          # elements per trip of the encode / decode grid (256 x 256 threads)
ABS_TRIP = 64 * 256           # ... of the absmax grid


def seg_table():
    """segments at odd offsets -> (segments, buffer length): 1 element, 257 elements, an empty
    segment, 1 002 elements ending at 1 265 (off a multiple of 4) and the three-trip segment; every
    non-empty segment has an element before and after it that belongs to no segment"""
    segs = [(3, 4), (5, 262), (262, 262), (263, 1265), (1273, 1273 + BIG)]
    n = 1273 + BIG + 5
    assert -(-BIG // ENC_TRIP) == 3 and -(-BIG // ABS_TRIP) == 9
    assert segs[3][1] % 4 != 0 and all(a % 2 == 1 for a, b in segs if b > a)
    inside = inside_mask(segs, n)
    for a, b in segs:
        if b > a:
            assert not bool(inside[a - 1]) and not bool(inside[b])
    return segs, n


def inside_mask(segs, n):
    m = torch.zeros(n, dtype=torch.bool)
    for a, b in segs:
        m[a:b] = True
    return m


def table_data(seed, place="none", scale=1.0):
    """Gaussian data on the segment table; `place` puts each segment's maximum at its first
    element, its last element, as a negative value only, or a value 1 000 x larger immediately
    outside either end"""
    segs, n = seg_table()
    x = torch.randn(n, generator=_gen(seed)) * scale
    for a, b in segs:
        if b <= a:
            continue
        mx = float(x[a:b].abs().max())
        if place == "first":
            x[a] = 3 * mx
        elif place == "last":
            x[b - 1] = 3 * mx
        elif place == "negative":
            x[a + (b - a) // 2] = -3 * mx
        elif place == "outside":
            x[a - 1], x[b] = 1000 * mx, -1000 * mx
        else:
            assert place == "none"
    return x, segs


def check_encode(dev, x, segs, codec, what, skip=()):
    """encode on `dev` against the oracle on the CPU: scales equal, payload bits equal inside every
    segment (but those in `skip`), zero bits outside all of them -> (payload, scales) of `dev` and
    of the oracle"""
    codec_ops, oracle = codec_mods()
    q, s = codec_ops.encode_segments(x.to(dev), segs, codec)
    qo, so = oracle.encode_segments(x, segs, codec)
    assert q.dtype == oracle.WIRE_DTYPE[codec] and tuple(q.shape) == (x.numel(),)
    assert s.dtype == torch.float32 and tuple(s.shape) == (len(segs),)
    keep = [k for k in range(len(segs)) if k not in skip]
    assert torch.equal(s.cpu()[keep], so[keep]), (what + " scales", s.cpu().tolist(), so.tolist())
    gb, ob = bits(q), bits(qo)
    for k in keep:
        a, b = segs[k]
        assert_bits(gb[a:b], ob[a:b], f"{what} payload of segment {k} [{a}, {b})")
    outside = ~inside_mask(segs, x.numel())
    assert not bool(gb[outside].any()), what + ": payload outside every segment is not zero"
    return q, s, qo, so


def oracle_sum(payloads, scales, segs, codec, weights, n):
    """the oracle's decode, weighted and accumulated in rank order in fp32 into zeros"""
    _, oracle = codec_mods()
    acc = torch.zeros(n)
    for q, s, w in zip(payloads, scales, weights):
        oracle.decode_segments_accumulate(acc, q, s, segs, codec, weight=w)
    return acc


def check_decode(dev, payloads, scales, segs, codec, weights, n, exact, fam):
    """codec_decode_sum into a sentinel-filled `out`, the payload elements outside every segment
    set to a sentinel as well: nothing outside the segments is written, two calls give the same
    bits, and inside the result equals the oracle's accumulation bit for bit (`exact`) or lies
    within world 2^-24 sum |w d| of the fp64 sum -> the result on the CPU"""
    codec_ops, oracle = codec_mods()
    inside = inside_mask(segs, n)
    payloads = [p.clone() for p in payloads]
    for p in payloads:
        p[~inside] = QSENT
    outs = []
    for _ in range(2):
        out = torch.full((n,), SENT, device=dev)
        codec_ops.decode_sum_segments(out, [p.to(dev) for p in payloads], [s.to(dev) for s in scales],
                                      segs, codec, weights)
        outs.append(out.cpu())
    got = outs[0]
    assert bool((got[~inside] == SENT).all()), fam + ": decode wrote outside the segments"
    assert_bits(outs[1], got, fam + ": a second decode of the same payloads")
    if exact:
        assert_bits(got[inside], oracle_sum(payloads, scales, segs, codec, weights, n)[inside], fam)
    else:
        w32 = torch.tensor(list(weights), dtype=torch.float32).double()
        ref = torch.zeros(n, dtype=torch.float64)
        mag = torch.zeros(n, dtype=torch.float64)
        for r, (q, s) in enumerate(zip(payloads, scales)):
            for (a, b), sk in zip(segs, s):
                d = oracle.decode(q[a:b], sk, codec)
                assert d.dtype == torch.float32
                ref[a:b] += w32[r] * d.double()
                mag[a:b] += (w32[r] * d.double()).abs()
        record(fam, got[inside], ref[inside], len(payloads) * U * mag[inside])
    return got


def run_table(dev, codec, place):
    """encode + decode (world 1, w = 1) of the segment table against the oracle"""
    x, segs = table_data(31, place)
    _, _, qo, so = check_encode(dev, x, segs, codec, f"table-{place}")
    check_decode(dev, [qo], [so], segs, codec, [1.0], x.numel(), True, f"decode table-{place}")


# rounding ties: the payload of k / K * 2^e for k = -K..K under round-half-to-even
TIE_PAYLOAD = {"int8_absmax": [-10, -8, -5, -2, 0, 2, 5, 8, 10],
               "fp16_absmax": [-100, -88, -75, -62, -50, -38, -25, -12, 0, 12, 25, 38, 50, 62, 75, 88, 100]}


def run_ties(dev, codec):
    """scale 2^e (e = -7, 0, 5), elements k/4 2^e (int8, L = 10) or k/8 2^e (fp16, L = 100):
    g / scale * L is exact in fp32 and every odd k is a tie"""
    _, oracle = codec_mods()
    K, L = (4, 10.0) if codec == "int8_absmax" else (8, 100.0)
    g = _gen(32)
    segs, parts, want, off = [], [torch.zeros(1)], [torch.zeros(1)], 1
    for e in (-7, 0, 5):
        kk = torch.arange(-K, K + 1).repeat(37)
        kk = kk[torch.randperm(kk.numel(), generator=g)]
        vals = (kk.double() / K * 2.0 ** e).float()
        v64 = vals.double() / 2.0 ** e * L
        assert torch.equal((vals / torch.tensor(2.0 ** e) * L).double(), v64), "bad case: not exact in fp32"
        tie = float(((v64 - v64.floor()) == 0.5).double().mean())
        assert tie >= 1 / 3, f"bad case: only {tie:.3f} of the elements are rounding ties"
        TIES[f"ties {codec} e={e}"] = tie
        segs.append((off, off + vals.numel()))
        parts += [vals, torch.zeros(1)]
        want += [torch.tensor(TIE_PAYLOAD[codec])[kk + K].float(), torch.zeros(1)]
        off += vals.numel() + 1
    x, want = torch.cat(parts), torch.cat(want).to(oracle.WIRE_DTYPE[codec])
    q, s, qo, so = check_encode(dev, x, segs, codec, "ties")
    assert torch.equal(so, torch.tensor([2.0 ** -7, 1.0, 32.0]))
    inside = inside_mask(segs, x.numel())        # (the oracle leaves the gaps uninitialised)
    assert_bits(qo[inside], want[inside], "ties: the oracle against the written-out half-to-even payload")
    assert_bits(q, want, "ties")
    check_decode(dev, [qo], [so], segs, codec, [1.0], x.numel(), True, "decode ties")


def run_magnitudes(dev, codec):
    """segment scales log-uniform over 1e-30 .. 1e30, and an all-zero segment (scale 0, zeros)"""
    g = _gen(33)
    exps = [-30.0, 30.0] + (torch.rand(10, generator=g) * 60 - 30).tolist()
    segs, parts, off = [], [], 0
    for e in exps + [None]:
        parts.append(torch.zeros(3))
        off += 3
        v = torch.zeros(301) if e is None else torch.randn(301, generator=g) * 10.0 ** e
        assert bool(torch.isfinite(v).all())
        segs.append((off, off + 301))
        parts.append(v)
        off += 301
    x = torch.cat(parts + [torch.zeros(2)])
    q, s, qo, so = check_encode(dev, x, segs, codec, "magnitudes")
    assert float(s[-1]) == 0.0 and not bool(bits(q)[segs[-1][0]:segs[-1][1]].any()), "all-zero segment"
    assert float(so[:-1].min()) < 1e-28 and float(so[:-1].max()) > 1e28
    check_decode(dev, [qo], [so], segs, codec, [1.0], x.numel(), True, "decode magnitudes")


SUBNORMAL = {"int8_absmax": [10, -3, 0, 0], "fp16_absmax": [100, -30, 5, 0]}


def run_subnormal(dev, codec):
    """a segment of subnormal gradients: a kernel that flushes them gives scale 0 and zeros"""
    _, oracle = codec_mods()
    x = torch.tensor([0.0, 1e-40, -3e-41, 5e-42, 0.0, 0.0])
    segs = [(1, 5)]
    assert 0 < float(x[1]) < 2.0 ** -126, "bad case: not subnormal on this host"
    want = torch.zeros(6)
    want[1:5] = torch.tensor(SUBNORMAL[codec]).float()
    q, s, qo, so = check_encode(dev, x, segs, codec, "subnormal")
    want = want.to(oracle.WIRE_DTYPE[codec])
    assert_bits(qo[1:5], want[1:5], "subnormal: the oracle against the written-out payload")
    assert_bits(q, want, "subnormal")
    check_decode(dev, [qo], [so], segs, codec, [1.0], 6, True, "decode subnormal")


def reference_weights(world):
    return codec_mods()[1].reference_weights(world)


def run_decode(dev, codec, world, weights, exact):
    """W ranks with differing payloads (the oracle's encodes of W Gaussian gradients of differing
    magnitude) on the segment table"""
    _, oracle = codec_mods()
    segs, n = seg_table()
    assert len(weights) == world
    if exact:
        assert all(math.frexp(w)[0] == 0.5 for w in weights), "bad case: a weight is no power of two"
    payloads, scales = [], []
    for r in range(world):
        x, _ = table_data(40 + r, scale=0.5 + 0.75 * r)
        q, s = oracle.encode_segments(x, segs, codec)
        payloads.append(q)
        scales.append(s)
    assert not torch.equal(payloads[0][segs[-1][0]:], payloads[-1][segs[-1][0]:]) or world == 1
    fam = f"codec_decode_sum {codec}"
    check_decode(dev, payloads, scales, segs, codec, weights, n, exact, fam)


NONFINITE_AT = {          # (segment, index): the 257-element segment (lane 13 of the second wave);
    "small": (1, 5 + 77),                 # the big one, where the thread that reads the value reads
    "big-first-trip": (4, 1273 + 100),    # eight finite ones after it; and its last element
    "big-last": (4, 1273 + BIG - 1),
}


def run_nonfinite(dev, codec, bad, where):
    """a NaN / +Inf / -Inf in one segment: that segment's scale is NaN / +Inf and after the decode
    every element of it is NaN whichever rank sent it; every other segment is bit-identical to the
    same buffer without the bad value (payload bits inside the poisoned segment are not compared)"""
    codec_ops, _ = codec_mods()
    x, segs = table_data(34)
    k, idx = NONFINITE_AT[where]
    a, b = segs[k]
    assert a <= idx < b
    n = x.numel()
    xb = x.clone()
    xb[idx] = bad
    q0, s0, _, _ = check_encode(dev, x, segs, codec, "clean")
    q1, s1, _, _ = check_encode(dev, xb, segs, codec, f"{bad} {where}", skip=(k,))
    q0, s0, q1, s1 = q0.cpu(), s0.cpu(), q1.cpu(), s1.cpu()
    if math.isnan(bad):
        assert math.isnan(float(s1[k])), f"scale of the segment with a NaN is {float(s1[k])!r}, not NaN"
    else:
        assert float(s1[k]) == math.inf, f"scale of the segment with {bad} is {float(s1[k])!r}, not +Inf"
    others = torch.ones(n, dtype=torch.bool)
    others[a:b] = False
    assert_bits(q1[others], q0[others], "payload of the other segments")
    clean = check_decode(dev, [q0, q0], [s0, s0], segs, codec, [1.0, 1.0], n, True, "decode clean")
    for qa, sa, qb, sb in ((q1, s1, q0, s0), (q0, s0, q1, s1)):
        out = torch.full((n,), SENT, device=dev)
        codec_ops.decode_sum_segments(out, [qa.to(dev), qb.to(dev)], [sa.to(dev), sb.to(dev)],
                                      segs, codec, [1.0, 1.0])
        got = out.cpu()
        nan = torch.isnan(got[a:b])
        assert bool(nan.all()), (f"{bad} {where}: {int((~nan).sum())} of {b - a} elements of the poisoned "
                                 f"segment are finite after the decode")
        assert_bits(got[others], clean[others], "decode of the other segments")


# ------------------------------------------------------------------ Adam
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAM_TRIP = 2048 * 256 * 4    # elements per trip of the capped grid's float4 loop
ADAM_BIG = 2 * ADAM_TRIP + 3 * 1024 + 3


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def adam_grad(n, t, seed):
    """log-uniform magnitudes over five decades, random signs; a seventh exactly zero: the
    elements 0 mod 14 at every step (their v stays 0 without weight decay) and one more residue
    that moves with the step (zero gradient on a non-zero v from step 2 on)"""
    g = _gen(seed * 100 + t)
    x = 10.0 ** (torch.rand(n, generator=g) * 5 - 5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    i = torch.arange(n)
    x[(i % 14 == 0) | (i % 14 == 1 + t % 13)] = 0.0
    return x.float()


def adam_ref(p0, m0, v0, g, b1, b2, eps, wd, ss, inv):
    """one step of the kernels' expression in fp64 from the fp32 state before the call; every
    scalar is the fp32 value the kernel receives.  -> ((m, Em), (v, Ev), (p, Ep)): references and
    bounds.  The kernel computes, each operation rounded once (u = 2^-24) unless contracted:

        gr = g + wd p                      Egr = u (|wd p| + |gr|)                  (0 without wd)
        m' = m + (1 - b1) (gr - m)         Em  = (1-b1) Egr + 2 u (1-b1) |gr - m| + u |m'|
        v' = b2 v + ((1 - b2) gr) gr       Ev  = 2 (1-b2) |gr| Egr + u (b2 v + 2 (1-b2) gr^2 + v')
        s  = sqrt(v')                      Es  = Ev / (sqrt(v') + sqrt(max(v' - Ev, 0))) + u s
        d  = s inv + eps                   Ed  = inv Es + u s inv + u d
        q  = (ss m') / d                   Eq  = (ss Em + u |ss m'| + |q| Ed) / (d - Ed) + u |q|
        p' = p - q                         Ep  = Eq + u |p'|

    (1 - b1, 1 - b2 are formed in fp32 by the kernel and taken as such here.)  The sqrt term is
    the exact worst case of sqrt over [v' - Ev, v' + Ev], valid also where Ev is not small against
    v' (g near -wd p).  Second-order terms are covered by a factor 1 + 2^-10 on every bound."""
    one = torch.tensor(1.0, dtype=torch.float32)
    omb1 = float(one - torch.tensor(b1, dtype=torch.float32))
    omb2 = float(one - torch.tensor(b2, dtype=torch.float32))
    p, m, v, gd = p0.double(), m0.double(), v0.double(), g.double()
    if wd != 0.0:
        gr = gd + wd * p
        Egr = U * ((wd * p).abs() + gr.abs())
    else:
        gr, Egr = gd, torch.zeros_like(gd)
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
    pr = p - q
    Ep = Eq + U * pr.abs()
    k = 1 + 2.0 ** -10
    return (mr, k * Em), (vr, k * Ev), (pr, k * Ep)


def ulp32(x):
    """the spacing of fp32 at |x|"""
    return 2.0 ** (math.frexp(x)[1] - 24)


def run_adam(o, dev, n, wd, dev_scal=False, offset=0, steps=5, seed=21):
    """`steps` Adam steps, each checked on its own against adam_ref; the buffers are views at
    `offset` floats into sentinel-filled allocations, which must stay untouched around them"""
    lr, b1, b2, eps = ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"]
    pad = 67

    def buf(init):
        big = torch.full((offset + n + pad,), SENT)
        big[offset:offset + n] = init
        big = big.to(dev)
        return big, big[offset:offset + n]
    P, p = buf(torch.randn(n, generator=_gen(seed)))
    M, m = buf(torch.zeros(n))
    V, v = buf(torch.zeros(n))
    G, g = buf(torch.zeros(n))
    scal = torch.zeros(3, device=dev) if dev_scal else None
    fam = ("adam_step_dev" if dev_scal else "adam_step") + (" wd" if wd else "")
    nzero = nzero_v = 0
    for t in range(1, steps + 1):
        gc = adam_grad(n, t, seed)
        g.copy_(gc)
        p0, m0, v0 = p.cpu().clone(), m.cpu().clone(), v.cpu().clone()
        if dev_scal:
            o.adam_step_dev(p, g, m, v, scal, lr, b1, b2, eps, wd)
            sc = scal.cpu()
            assert float(sc[0]) == float(t)
            ss64, inv64 = lr / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t)
            assert abs(float(sc[1]) - ss64) <= ulp32(ss64), ("step_size", t, float(sc[1]), ss64)
            assert abs(float(sc[2]) - inv64) <= ulp32(inv64), ("inv_sqrt_bc2", t, float(sc[2]), inv64)
            ss, inv = float(sc[1]), float(sc[2])
        else:
            ss64, inv64 = lr / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t)
            o.adam_step(p, g, m, v, b1, b2, eps, wd, ss64, inv64)
            ss, inv = f32(ss64), f32(inv64)
        (mr, Em), (vr, Ev), (pr, Ep) = adam_ref(p0, m0, v0, gc, f32(b1), f32(b2), f32(eps), f32(wd), ss, inv)
        p1, m1, v1 = p.cpu(), m.cpu(), v.cpu()
        record(fam + " m", m1, mr, Em)
        record(fam + " v", v1, vr, Ev)
        record(fam + " p", p1, pr, Ep)
        assert torch.equal(g.cpu(), gc), "the gradient was written"
        zg = gc == 0
        nzero += int(zg.sum())
        if wd == 0.0:
            # zero gradient on zero moments: nothing moves, not even by the eps term
            still = zg & (m0 == 0) & (v0 == 0)
            nzero_v += int(still.sum())
            assert_bits(p1[still], p0[still], "p where g = m = v = 0")
            assert not bool(m1[still].any()) and not bool(v1[still].any())
    if n >= 14:
        assert abs(nzero / (steps * n) - 1 / 7) < 0.02, "bad case: not a seventh of the gradients is zero"
    assert wd != 0.0 or nzero_v > 0, "bad case: no zero gradient on v = 0"
    for name, big in (("p", P), ("m", M), ("v", V), ("g", G)):
        b = big.cpu()
        assert bool((b[:offset] == SENT).all()) and bool((b[offset + n:] == SENT).all()), (
            f"{name}: written outside the view")


# ------------------------------------------------------------------ weight_pack
# (kind, Cout, Cin, taps or sub-positions, dgrad)
PACK = [
    ("conv", 32, 3, 9, True),          # the image layer: CinW = 8, five pad channels
    ("conv", 32, 64, 9, False),        # no data-gradient copy
    ("conv", 32, 96, 9, True),
    ("conv", 32, 32, 27, True),        # 27 taps: column tiles 10 wide, the last one partial
    ("conv", 32, 3, 27, True),
    ("convT", 32, 64, 4, True),
    ("convT", 16, 32, 8, True),
    ("conv", 40, 24, 9, True),         # Cout, Cin no multiples of 32 (CinW = Cin: no pads)
]
PACK_TILE = 9216              # fp32 elements per workgroup step (32 x 32 channels x 9 taps)


def pack_case(kind, cout, cin, T, dgrad, seed):
    """-> (w, fwd reference, dgrad reference or None): the layouts of csrc/misc.hip written out
    as permutations; pads (ci >= Cin of the conv fwd copy) hold the sentinel"""
    if kind == "conv":
        w, tie = rounding_mix((cout, cin, T), seed)                   # OIHW, taps flattened
        cinw = (cin + 7) // 8 * 8
        fwd = torch.full((cout, T, cinw), SENT, dtype=torch.bfloat16)
        fwd[:, :, :cin] = w.permute(0, 2, 1).bfloat16()               # [co][tap][ci]
        dg = w.flip(2).permute(1, 2, 0).bfloat16().contiguous()       # [ci][T-1-tap][co]
    else:
        w, tie = rounding_mix((cin, cout, T), seed)                   # IOHW, sub-positions flattened
        cinw = cin
        fwd = w.permute(2, 1, 0).bfloat16().contiguous()              # [(sub, co)][ci]
        dg = w.permute(0, 2, 1).bfloat16().contiguous()               # [ci][(sub, co)]
    TIES["weight_pack bf16 ties"] = min(TIES.get("weight_pack bf16 ties", 1.0), tie)
    return w, fwd, (dg if dgrad else None), cinw


def run_weight_pack(o, dev, max_elems=None):
    """every entry of PACK in ONE launch (blockIdx.y = the entry), max_elems from the largest as
    UNetEngine.pack_weights derives it, or 1 (one workgroup per entry loops over all its tiles)"""
    cases = [pack_case(*c, seed=50 + i) for i, c in enumerate(PACK)]
    largest = max(c[0].numel() for c in cases)
    assert largest > 2 * PACK_TILE, "bad case: the largest entry fits two workgroup steps"
    keep, rows = [], []
    for (kind, cout, cin, T, dgrad), (w, fwd, dg, cinw) in zip(PACK, cases):
        src = w.contiguous().to(dev)
        dfwd = torch.full(fwd.shape, SENT, dtype=torch.bfloat16, device=dev)
        ddg = torch.full(dg.shape, SENT, dtype=torch.bfloat16, device=dev) if dgrad else None
        keep.append((src, dfwd, ddg))
        rows.append([src.data_ptr(), dfwd.data_ptr(), ddg.data_ptr() if dgrad else 0,
                     (0 if kind == "conv" else 1) | (cout << 32), cin | (T << 32), cinw | (cout << 32)])
    ent = torch.tensor(rows, dtype=torch.int64).to(dev)
    o.weight_pack(ent, len(rows), largest if max_elems is None else max_elems)
    for i, ((src, dfwd, ddg), (w, fwd, dg, _)) in enumerate(zip(keep, cases)):
        assert_bits(src, w, f"entry {i} {PACK[i]}: the source was written")
        assert_bits(dfwd, fwd, f"entry {i} {PACK[i]} fwd")
        if dg is not None:
            assert_bits(ddg, dg, f"entry {i} {PACK[i]} dgrad")


# ------------------------------------------------------------------ to_nhwc_bf16
def run_to_nhwc(o, dev, C, cpad, dtype, layout, dims):
    """bit-exact against .bfloat16() of the permuted input, channels zero-padded to Cp"""
    shape = (2, C, 5, 7) if dims == 2 else (2, C, 3, 5, 7)
    x, tie = rounding_mix(shape, 60 + C)
    TIES["to_nhwc_bf16 bf16 ties (fp32 inputs)"] = min(TIES.get("to_nhwc_bf16 bf16 ties (fp32 inputs)", 1.0), tie)
    x = x.to(dtype)
    Cp = (C + cpad - 1) // cpad * cpad
    perm = (0, 2, 3, 1) if dims == 2 else (0, 2, 3, 4, 1)
    ref = torch.zeros(tuple(x.permute(perm).shape[:-1]) + (Cp,), dtype=torch.bfloat16)
    ref[..., :C] = x.bfloat16().permute(perm)
    xin = x.to(dev)
    if layout == "channels_last":
        xin = xin.contiguous(memory_format=torch.channels_last if dims == 2 else torch.channels_last_3d)
        assert C == 1 or not xin.is_contiguous()
    else:
        assert xin.is_contiguous()
    y = o.to_nhwc_bf16(xin, cpad)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == tuple(ref.shape) and y.is_contiguous()
    assert_bits(y, ref, f"to_nhwc_bf16 C={C} cpad={cpad} {dtype} {layout} {dims}-D")
    return Cp


# ------------------------------------------------------------------ bindings
def seg_tensor(segs, dev):
    return torch.tensor([v for s in segs for v in s], dtype=torch.int64, device=dev)


def run_empty(o, dev):
    """calls with nothing to do return before any launch"""
    x = torch.randn(10).to(dev)
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    s = o.codec_absmax(x, none)
    assert s.dtype == torch.float32 and tuple(s.shape) == (0,)
    for cid, dt in ((0, torch.float16), (1, torch.int8)):
        q = o.codec_encode(x, none, s, cid)
        assert q.dtype == dt and tuple(q.shape) == (10,) and not bool(q.cpu().any())
        e = torch.zeros(0, device=dev)
        q0 = o.codec_encode(e, none, s, cid)
        assert q0.dtype == dt and q0.numel() == 0
        out = torch.full((10,), SENT, device=dev)
        o.codec_decode_sum(out, torch.zeros(2, 10, dtype=dt, device=dev), torch.zeros(2, 0, device=dev),
                           torch.ones(2, device=dev), none, cid)
        assert bool((out.cpu() == SENT).all())
        o.codec_decode_sum(e, torch.zeros(2, 0, dtype=dt, device=dev), torch.zeros(2, 0, device=dev),
                           torch.ones(2, device=dev), none, cid)
    e = [torch.zeros(0, device=dev) for _ in range(4)]
    o.adam_step(*e, 0.9, 0.999, 1e-8, 0.0, 1e-3, 1.0)
    scal = torch.zeros(3, device=dev)
    o.adam_step_dev(*e, scal, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert float(scal[0]) == 1.0
    o.weight_pack(torch.zeros(0, 6, dtype=torch.int64, device=dev), 0, 1)
    y = o.to_nhwc_bf16(torch.zeros(0, 3, 5, 7, device=dev), 8)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (0, 5, 7, 8)


def binding_calls(o, dev):
    """name -> a call the GPU bindings must refuse (TORCH_CHECK) before any launch"""
    n = 16
    f = lambda *s, dt=torch.float32, d=dev: torch.zeros(*s, dtype=dt, device=d)
    strided = lambda: f(2 * n)[::2]
    seg = lambda d=dev: seg_tensor([(0, 8), (8, 16)], d)
    adam = lambda p=None, g=None, m=None, v=None: o.adam_step(
        f(n) if p is None else p, f(n) if g is None else g, f(n) if m is None else m,
        f(n) if v is None else v, 0.9, 0.999, 1e-8, 0.0, 1e-3, 1.0)
    adam_dev = lambda p=None, g=None, scal=None: o.adam_step_dev(
        f(n) if p is None else p, f(n) if g is None else g, f(n), f(n),
        f(3) if scal is None else scal, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    dec = lambda q=None, s=None, w=None, sg=None, codec=1, out=None: o.codec_decode_sum(
        f(n) if out is None else out, f(2, n, dt=torch.int8) if q is None else q,
        f(2, 2) if s is None else s, f(2) if w is None else w, seg() if sg is None else sg, codec)
    return {
        "adam_step p strided": lambda: adam(p=strided()),
        "adam_step g strided": lambda: adam(g=strided()),
        "adam_step m strided": lambda: adam(m=strided()),
        "adam_step v strided": lambda: adam(v=strided()),
        "adam_step g on the host": lambda: adam(g=f(n, d="cpu")),
        "adam_step m fp64": lambda: adam(m=f(n, dt=torch.float64)),
        "adam_step g shorter": lambda: adam(g=f(n - 1)),
        "adam_step_dev p strided": lambda: adam_dev(p=strided()),
        "adam_step_dev g strided": lambda: adam_dev(g=strided()),
        "adam_step_dev g on the host": lambda: adam_dev(g=f(n, d="cpu")),
        "adam_step_dev scal on the host": lambda: adam_dev(scal=f(3, d="cpu")),
        "codec_absmax seg int32": lambda: o.codec_absmax(f(n), seg().int()),
        "codec_absmax seg on the host": lambda: o.codec_absmax(f(n), seg("cpu")),
        "codec_absmax seg odd": lambda: o.codec_absmax(f(n), seg()[:3]),
        "codec_absmax x fp64": lambda: o.codec_absmax(f(n, dt=torch.float64), seg()),
        "codec_absmax x strided": lambda: o.codec_absmax(strided(), seg()),
        "codec_encode scales short": lambda: o.codec_encode(f(n), seg(), f(1), 1),
        "codec_encode scales fp64": lambda: o.codec_encode(f(n), seg(), f(2, dt=torch.float64), 1),
        "codec_encode scales on the host": lambda: o.codec_encode(f(n), seg(), f(2, d="cpu"), 1),
        "codec_encode codec 2": lambda: o.codec_encode(f(n), seg(), f(2), 2),
        "codec_decode_sum q int8 for fp16": lambda: dec(codec=0),
        "codec_decode_sum q fp16 for int8": lambda: dec(q=f(2, n, dt=torch.float16)),
        "codec_decode_sum q short": lambda: dec(q=f(2, n - 1, dt=torch.int8)),
        "codec_decode_sum q strided": lambda: dec(q=f(2, 2 * n, dt=torch.int8)[:, ::2]),
        "codec_decode_sum scales [world] only": lambda: dec(s=f(2)),
        "codec_decode_sum scales fp64": lambda: dec(s=f(2, 2, dt=torch.float64)),
        "codec_decode_sum w short": lambda: dec(w=f(1)),
        "codec_decode_sum w fp64": lambda: dec(w=f(2, dt=torch.float64)),
        "codec_decode_sum w on the host": lambda: dec(w=f(2, d="cpu")),
        "codec_decode_sum seg int32": lambda: dec(sg=seg().int()),
        "codec_decode_sum out strided": lambda: dec(out=strided()),
        "weight_pack entries int32": lambda: o.weight_pack(f(1, 6, dt=torch.int32), 1, 1),
        "weight_pack entries short": lambda: o.weight_pack(f(1, 5, dt=torch.int64), 1, 1),
    }


BINDING_NAMES = list(binding_calls(None, "cpu"))      # (the calls are built lazily: none runs here)
