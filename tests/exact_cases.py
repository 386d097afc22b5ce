"""Bit-exact integer cases for the conv / convT / weight-gradient kernels, written once and run
on both kernel sets: ``test_kernels_exact_gpu.py`` (the gfx950 kernels) and its
``test_kernels_exact_cpu.py`` mirror (the C++ kernels of ``csrc/cpu_ref.cpp``).

The method.  These kernels are linear with fp32 accumulation.  Fed small integers (ternary
{-1, 0, +1} activations and weights, integer biases, BatchNorm constants that are small powers
of two or integers), every product and every partial sum is an integer multiple of a known
power of two ``q`` (the *quantum*) with magnitude below 2^24 q: exact in fp32 in ANY summation
order, with or without fused multiply-adds.  A bf16 output whose magnitude is at most 256 q is
stored exactly.  So the kernel must equal an fp64 reference bit for bit (``torch.equal``) and
a single wrong element anywhere fails the test — no tolerance to choose.

``assert_exact`` first asserts that precondition ON THE REFERENCE ALONE (a case that breaks it
is a bad case, not a pass), then equality; on failure it reports the number of wrong elements,
the first few (n, d, h, w, c) indices and their position inside the 16 x 16 pixel tile.

Every input is generated on the CPU from a seed (identical on both devices) and every reference
is computed on the CPU in fp64 with ``F.conv2d`` / ``F.conv3d`` / ``F.conv_transpose2d/3d`` and
autograd.

Worst ``max|ref| / q`` over the cases of ``test_kernels_exact_gpu.py`` per family, from the
generators run on the CPU for every case (bf16 outputs: the bound is 256; fp32 outputs and
statistics rows: the bound is 2^24 = 16 777 216; the sum of the magnitudes of a row's terms is
held to the same bound by ``assert_exact``):

    family            bf16 outputs   fp32 outputs   statistics / partial rows
    conv3_fwd              131             -            6 008 281  (sum y^2)
    conv3_dgrad             86             -              331 682
    conv3d_fwd             123             -            4 075 751  (sum y^2)
    conv3_wgrad             80  (dY)    13 792               -
    conv3d_wgrad             -           1 746               -
    conv3_bwd32             38             422              7 224
    convt_fwd              101             -                 -
    convt_dgrad             67             -                2 512
    convt_wgrad              -             184               -
    convt_bwd_fused         37             224              2 032

(``WORST`` collects these figures while the cases run.)
"""
import math

import torch
import torch.nn.functional as F

F32_EXACT = float(2 ** 24)


def ops():
    from ddlpc.ops import _ext
    return _ext.ops()


WORST = {}            # family -> worst max|ref| / q seen by assert_exact (for the docs)


# ------------------------------------------------------------------ generators (CPU, seeded)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def tern(shape, density, seed):
    """bf16 tensor with values in {-1, 0, +1}; P(non-zero) = density"""
    g = _gen(seed)
    nz = torch.rand(shape, generator=g) < density
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (nz * sign).to(torch.bfloat16)


def int_bias(C, seed):
    """integer bias in [-3, 3] (fp32)"""
    return torch.randint(-3, 4, (C,), generator=_gen(seed)).float()


def bn_prologue(C, seed):
    """BN-apply + ReLU prologue constants: scale cycles through {1, 2, -1, 0.5} (negative and
    fractional channels present), integer shift in [-1, 1].  On ternary inputs the
    pre-activation is exactly 0 for a large share of the elements."""
    scale = torch.tensor([1.0, 2.0, -1.0, 0.5]).repeat((C + 3) // 4)[:C].contiguous()
    shift = torch.randint(-1, 2, (C,), generator=_gen(seed)).float()
    return scale, shift


def bn_stats4(C, seed):
    """[mean | invstd | scale | shift] x C with integer mean in [-1, 1], invstd in {0.5, 1, 2},
    scale in {1, 2, -1, 0.5}, integer shift in [-1, 1]"""
    g = _gen(seed)
    mean = torch.randint(-1, 2, (C,), generator=g).float()
    invstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    scale, shift = bn_prologue(C, seed + 1)
    return torch.stack([mean, invstd, scale, shift]).contiguous()


def bn_coefs(C, seed):
    """dY-prologue coefficients [k | m1 | m2] x C: k in {0.5, 1, 2}, integer m1 in [-2, 2],
    m2 in {0, +-0.5, +-1}"""
    g = _gen(seed)
    k = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    m1 = torch.randint(-2, 3, (C,), generator=g).float()
    m2 = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0])[torch.randint(0, 5, (C,), generator=g)]
    return torch.stack([k, m1, m2]).contiguous()


def pack(o, w, dev):
    """pack an OIHW(D) / IOHW(D) fp32 weight with the library's packer on `dev`"""
    from ddlpc.ops.fused_unet import _ConvPack
    conv = torch.nn.Module()
    conv.weight = torch.nn.Parameter(w.to(dev).contiguous())
    kind = 0 if w.shape[-1] == 3 else 1
    pk = _ConvPack(conv, kind, True)
    ent = torch.tensor([pk.entry()], dtype=torch.int64, device=dev)
    o.weight_pack(ent, 1, pk.numel())
    return pk


def cf(x):            # channel-last [N, S..., C] -> channel-first fp64
    return x.double().permute(0, x.dim() - 1, *range(1, x.dim() - 1))


def cl(x):            # channel-first -> channel-last
    return x.permute(0, *range(2, x.dim()), 1).contiguous()


def _chan(v, G, like):
    """[C] or [G][C] per-channel constants broadcast over a channel-last tensor of G groups"""
    v = v.double()
    if v.dim() == 2:
        n = like.shape[0] // G
        return v.repeat_interleave(n, 0).reshape(like.shape[0], *([1] * (like.dim() - 2)), -1)
    return v


def act64(x, scale, shift, G=1):
    """relu(x * scale + shift) in fp64 on a channel-last tensor"""
    xd = x.double()
    return torch.relu(xd * _chan(scale, G, xd) + _chan(shift, G, xd))


def conv_ref(xcl64, w64, bias=None):
    x = xcl64.permute(0, xcl64.dim() - 1, *range(1, xcl64.dim() - 1))
    fn = F.conv2d if w64.dim() == 4 else F.conv3d
    return cl(fn(x, w64, None if bias is None else bias.double(), padding=1))


def dgrad_ref(dycl64, w64):
    """data gradient of the 'same' conv with OIHW(D) weight w: channel-last [.., Cin]"""
    dy = dycl64.permute(0, dycl64.dim() - 1, *range(1, dycl64.dim() - 1))
    fn = F.conv_transpose2d if w64.dim() == 4 else F.conv_transpose3d
    return cl(fn(dy, w64, padding=1))


def wgrad_ref(dycl64, xcl64):
    """weight gradient of the 'same' conv by autograd: OIHW(D) fp64"""
    dims = xcl64.dim() - 2
    x = xcl64.permute(0, xcl64.dim() - 1, *range(1, xcl64.dim() - 1))
    dy = dycl64.permute(0, dycl64.dim() - 1, *range(1, dycl64.dim() - 1))
    w = torch.zeros(dy.shape[1], x.shape[1], *([3] * dims), dtype=torch.float64, requires_grad=True)
    fn = F.conv2d if dims == 2 else F.conv3d
    (g,) = torch.autograd.grad(fn(x, w, padding=1), w, dy)
    return g


def bnb_terms(dA64, y, s4, G=1):
    """(dyh, xhat) of the BatchNorm backward: dyh = dA [y * scale + shift > 0] (STRICT),
    xhat = (y - mean) * invstd; s4 [4][C] or [G][4][C]"""
    yd = y.double()
    s = s4.reshape(G, 4, -1) if G > 1 else s4
    row = (lambda r: s[:, r]) if G > 1 else (lambda r: s[r])
    a = yd * _chan(row(2), G, yd) + _chan(row(3), G, yd)
    dyh = torch.where(a > 0, dA64, torch.zeros_like(dA64))
    xh = (yd - _chan(row(0), G, yd)) * _chan(row(1), G, yd)
    return dyh, xh


def rows_ref(terms):
    """per-channel sums of channel-last terms -> ([C] sum, [C] sum of magnitudes)"""
    C = terms.shape[-1]
    t = terms.reshape(-1, C)
    return t.sum(0), t.abs().sum(0)


# ------------------------------------------------------------------ the assertion
def _report(bad, shape, what, got, ref):
    idx = bad.nonzero()
    lines = [f"{what}: {idx.shape[0]} of {bad.numel()} elements differ; first (index) got / ref:"]
    for i in idx[:8].tolist():
        pos = ""
        if len(shape) >= 4:          # channel-last activation: [N, (D,) H, W, C]
            h, w = i[-3], i[-2]
            pos = f"  tile ({h // 16}, {w // 16}) row {h % 16} col {w % 16}"
        lines.append(f"  {tuple(i)} {float(got[tuple(i)])!r} / {float(ref[tuple(i)])!r}{pos}")
    return "\n".join(lines)


def assert_exact(got, ref64, what, kind="bf16", q=1.0, abs_sum=None, family=None):
    """got == ref64 bit for bit, after checking on the reference alone that the case is exact:
    every value a multiple of q; bf16 outputs |ref| <= 256 q; fp32 outputs and statistics rows
    |ref| < 2^24 q and (abs_sum: the sum of the magnitudes of the terms) < 2^24 q."""
    ref64 = ref64.double().cpu()
    r = ref64 / q
    assert torch.equal(r, r.round()), f"{what}: bad case, reference is not a multiple of q={q}"
    m = float(r.abs().max()) if r.numel() else 0.0
    if kind == "bf16":
        assert m <= 256, f"{what}: bad case, max|ref|/q = {m} > 256 (not exact in bf16)"
        assert got.dtype == torch.bfloat16, (what, got.dtype)
    else:
        s = float((abs_sum.double() / q).max()) if abs_sum is not None else m
        assert m < F32_EXACT and s < F32_EXACT, f"{what}: bad case, {m} / {s} not below 2^24"
    if family is not None:
        key = (family, kind)
        WORST[key] = max(WORST.get(key, 0.0), m)
    g = got.detach().double().cpu()
    assert g.shape == ref64.shape, (what, tuple(g.shape), tuple(ref64.shape))
    if not torch.equal(g, ref64):
        bad = g != ref64
        raise AssertionError(_report(bad, tuple(g.shape), what, g, ref64))


def assert_bound(got, ref64, S64, what):
    """per-element bound for the non-linear kernels (bf16 outputs):
    |got - ref| <= 2^-8 |ref| + 2^-20 S, S = the reference on the magnitudes of the inputs and
    coefficients.  2^-9 |ref| is the round-to-nearest bf16 store; the factor 2 accepts a value
    that fp32 error moved onto the adjacent bf16 value; 2^-20 S bounds the fp32 evaluation
    error of a few dozen operations with cancellation."""
    g = got.detach().double().cpu()
    ref64, S64 = ref64.double().cpu(), S64.double().cpu()
    assert g.shape == ref64.shape, (what, tuple(g.shape), tuple(ref64.shape))
    bad = (g - ref64).abs() > 2.0 ** -8 * ref64.abs() + 2.0 ** -20 * S64
    if bool(bad.any()):
        raise AssertionError(_report(bad, tuple(g.shape), what, g, ref64))


# ------------------------------------------------------------------ case runners
# Each runner builds the inputs of one case from its parameters, calls the operator on `dev`
# and asserts every output exactly; it returns the operator's last_path().
def _shape(c):
    return (c["N"],) + ((c["D"],) if c.get("D") else ()) + (c["H"], c["W"])


def run_conv3_fwd(o, dev, c):
    """conv3_fwd forward: Y1 / Y2 (split at co1) with bias and the X1 / X2 prologues, and the
    statistics rows (per-channel sum y, sum y^2 of the fp32 outputs)."""
    sp, C1, C2, Cout = _shape(c), c["C1"], c.get("C2", 0), c["Cout"]
    dims, seed, d = len(sp) - 1, c.get("seed", 1), c.get("dens", 0.5)
    G = c.get("groups", 0)
    img = c.get("img", False)                      # 3 real channels of an 8-channel padded input
    x1 = tern(sp + (C1,), d, seed)
    if img:
        x1[..., 3:] = 0
    x2 = tern(sp + (C2,), d, seed + 1) if C2 else None
    w = tern((Cout, C1 + C2) + (3,) * dims, d, seed + 2).float()
    bias = int_bias(Cout, seed + 3) if c.get("bias") else None
    q, a1, a2 = 1.0, x1.double(), x2.double() if C2 else None
    ps = sh = ps2 = sh2 = None
    if c.get("pro"):
        if G > 1:
            s4g = torch.stack([bn_stats4(C1, seed + 10 + g) for g in range(G)]).contiguous()
            ps, sh = s4g[:, 2], s4g[:, 3]
        else:
            ps, sh = bn_prologue(C1, seed + 4)
        a1, q = act64(x1, ps, sh, max(G, 1)), 0.5
    if c.get("pro2"):
        ps2, sh2 = bn_prologue(C2, seed + 5)
        a2, q = act64(x2, ps2, sh2), 0.5
    ref = conv_ref(torch.cat([a1, a2], -1) if C2 else a1, w.double(), bias)
    pk = pack(o, w, dev)
    co1 = c.get("co1", 0)
    t = lambda v: None if v is None else v.to(dev)
    if G > 1 and ps is not None:
        s4d = s4g.to(dev)
        psd, shd = s4d[:, 2], s4d[:, 3]
    else:
        psd, shd = t(ps), t(sh)
    y1, y2, st = o.conv3_fwd(t(x1), t(x2), pk.fwd, t(bias), psd, shd, Cout, co1, True, t(ps2), t(sh2),
                             None, None, G)
    path = o.last_path()
    fam = c.get("family", "conv3_fwd")
    if co1:
        assert_exact(y1, ref[..., :co1], "Y1", q=q, family=fam)
        assert_exact(y2, ref[..., co1:], "Y2", q=q, family=fam)
    else:
        assert y2.numel() == 0
        assert_exact(y1, ref, "Y", q=q, family=fam)
    s1, a1s = rows_ref(ref)
    s2, _ = rows_ref(ref * ref)
    if G > 1:
        # group-major rows [groups][R][2][Cout]
        rows = st.double().reshape(G, -1, 2, Cout).sum(1).cpu()
        rg = ref.reshape(G, -1, Cout)
        assert_exact(rows[:, 0], rg.sum(1), "stats sum rows", "rows", q, rg.abs().sum(1), fam)
        assert_exact(rows[:, 1], (rg * rg).sum(1), "stats sum^2 rows", "rows", q * q, family=fam)
    else:
        rows = st.double().sum(0)
        assert_exact(rows[0], s1, "stats sum row", "rows", q, a1s, fam)
        assert_exact(rows[1], s2, "stats sum^2 row", "rows", q * q, family=fam)
    return path


def run_conv3_dgrad(o, dev, c):
    """conv3_fwd as the data gradient (pk.dgrad): dX1 / dX2; with bnb: dA and both partial-row
    sums of the BatchNorm backward (sum dyh, sum dyh * xhat); else the statistics rows, whose
    sum^2 row the 96-channel resident variant documents as zeros."""
    sp, Cf, Cdy = _shape(c), c["Cin"], c["Cout"]     # the forward conv: Cin -> Cout
    dims, seed, d = len(sp) - 1, c.get("seed", 2), c.get("dens", 0.5)
    G = c.get("groups", 0)
    w = tern((Cdy, Cf) + (3,) * dims, d, seed).float()
    dy = tern(sp + (Cdy,), d, seed + 1)
    ref = dgrad_ref(dy.double(), w.double())
    pk = pack(o, w, dev)
    co1 = c.get("co1", 0)
    fam = c.get("family", "conv3_dgrad")
    if c.get("bnb"):
        y = tern(sp + (Cf,), 0.6, seed + 2)
        if G > 1:
            s4 = torch.stack([bn_stats4(Cf, seed + 10 + g) for g in range(G)]).contiguous()
        else:
            s4 = bn_stats4(Cf, seed + 3)
        dA, _, part = o.conv3_fwd(dy.to(dev), None, pk.dgrad, None, None, None, Cf, 0, False, None, None,
                                  y.to(dev), s4.to(dev), G)
        path = o.last_path()
        assert_exact(dA, ref, "dA", family=fam)
        dyh, xh = bnb_terms(ref, y, s4, max(G, 1))
        Gn = max(G, 1)
        rows = part.double().reshape(Gn, -1, 2, Cf).sum(1).cpu()
        t1, t2 = dyh.reshape(Gn, -1, Cf), (dyh * xh).reshape(Gn, -1, Cf)
        assert_exact(rows[:, 0], t1.sum(1), "BN rows sum dyh", "rows", 1.0, t1.abs().sum(1), fam)
        assert_exact(rows[:, 1], t2.sum(1), "BN rows sum dyh*xhat", "rows", 0.5, t2.abs().sum(1), fam)
        return path
    dx1, dx2, st = o.conv3_fwd(dy.to(dev), None, pk.dgrad, None, None, None, Cf, co1, True)
    path = o.last_path()
    if co1:
        assert_exact(dx1, ref[..., :co1], "dX1", family=fam)
        assert_exact(dx2, ref[..., co1:], "dX2", family=fam)
    else:
        assert_exact(dx1, ref, "dX", family=fam)
    rows = st.double().sum(0)
    s1, a1s = rows_ref(ref)
    assert_exact(rows[0], s1, "stats sum row", "rows", 1.0, a1s, fam)
    if path.startswith("conv3_fwd:res:v7"):
        assert torch.count_nonzero(rows[1]) == 0          # (documented: ops.h ConvFwdArgs::stats)
    else:
        assert_exact(rows[1], rows_ref(ref * ref)[0], "stats sum^2 row", "rows", family=fam)
    return path


def run_conv3_wgrad(o, dev, c):
    """conv3_wgrad: the whole fp32 dW, with the X1 / X2 prologues, the dY prologue (and the dY
    it stores with dy_out), BN groups, and the image layer's zero padding channels."""
    sp, C1, C2, Cout = _shape(c), c["C1"], c.get("C2", 0), c["Cout"]
    dims, seed, d = len(sp) - 1, c.get("seed", 3), c.get("dens", 0.5)
    G = c.get("groups", 0)
    img = c.get("img", False)
    x1 = tern(sp + (C1,), d, seed)
    if img:
        x1[..., 3:] = 0
    x2 = tern(sp + (C2,), d, seed + 1) if C2 else None
    dy = tern(sp + (Cout,), d, seed + 2)              # dY, or dA with the dY prologue
    q, a1, a2 = 1.0, x1.double(), x2.double() if C2 else None
    ps = sh = ps2 = sh2 = None
    if c.get("pro"):
        if G > 1:
            s4g = torch.stack([bn_stats4(C1, seed + 10 + g) for g in range(G)]).contiguous()
            ps, sh = s4g[:, 2], s4g[:, 3]
        else:
            ps, sh = bn_prologue(C1, seed + 4)
        a1, q = act64(x1, ps, sh, max(G, 1)), 0.5
    if c.get("pro2"):
        ps2, sh2 = bn_prologue(C2, seed + 5)
        a2, q = act64(x2, ps2, sh2), 0.5
    dy64 = dy.double()
    t = lambda v: None if v is None else v.to(dev)
    kw, dy_out = {}, None
    fam = c.get("family", "conv3_wgrad")
    if c.get("dypro"):
        y, s4, coefs = tern(sp + (Cout,), 0.6, seed + 6), bn_stats4(Cout, seed + 7), bn_coefs(Cout, seed + 8)
        dyh, xh = bnb_terms(dy64, y, s4)
        dy64 = coefs[0].double() * (dyh - coefs[1].double() - xh * coefs[2].double())
        q *= 0.125                                    # k, invstd and m2 are multiples of 1/2
        kw = dict(dy_y=y.to(dev), dy_s4=s4.to(dev), dy_coefs=coefs.to(dev))
        if c.get("dyout"):
            dy_out = torch.full(sp + (Cout,), 7.0, dtype=torch.bfloat16, device=dev)
            kw["dy_out"] = dy_out
    if img:
        kw["cin_real"] = 3
    if G > 1:
        kw["groups"] = G
        s4d = s4g.to(dev)
        psd, shd = s4d[:, 2], s4d[:, 3]
    else:
        psd, shd = t(ps), t(sh)
    xin = torch.cat([a1, a2], -1) if C2 else a1
    ref = wgrad_ref(dy64, xin)
    npix = math.prod(sp)
    bound = torch.tensor(npix * float(dy64.abs().max()) * float(xin.abs().max()))
    dw = o.conv3_wgrad(t(dy), t(x1), t(x2), psd, shd, None, t(ps2), t(sh2), **kw)
    path = o.last_path()
    assert_exact(dw, ref, "dW", "f32", q, bound, fam)
    if img:
        assert torch.count_nonzero(dw[:, 3:]) == 0    # the padded input channels: exactly 0
    if dy_out is not None:
        assert_exact(dy_out, dy64, "stored dY", q=0.125, family=fam)
    return path


def run_conv3_bwd32(o, dev, c):
    """conv3_bwd32: dA, the BN1 partial rows and dW of the fused 32-channel backward."""
    sp, C = _shape(c), 32
    seed, d, G = c.get("seed", 4), c.get("dens", 0.5), c.get("groups", 0)
    Gn = max(G, 1)
    y = tern(sp + (C,), 0.6, seed)
    dy = tern(sp + (C,), d, seed + 1)
    w = tern((C, C, 3, 3), d, seed + 2).float()
    s4 = (torch.stack([bn_stats4(C, seed + 10 + g) for g in range(G)]).contiguous() if G > 1
          else bn_stats4(C, seed + 3))
    pk = pack(o, w, dev)
    dA, part, dW = o.conv3_bwd32(dy.to(dev), y.to(dev), s4.to(dev), pk.dgrad, None, G)
    path = o.last_path()
    fam = "conv3_bwd32"
    dA64 = dgrad_ref(dy.double(), w.double())
    assert_exact(dA, dA64, "dA", family=fam)
    dyh, xh = bnb_terms(dA64, y, s4, Gn)
    rows = part.double().reshape(Gn, -1, 2, C).sum(1).cpu()
    t1, t2 = dyh.reshape(Gn, -1, C), (dyh * xh).reshape(Gn, -1, C)
    assert_exact(rows[:, 0], t1.sum(1), "BN rows sum dyh", "rows", 1.0, t1.abs().sum(1), fam)
    assert_exact(rows[:, 1], t2.sum(1), "BN rows sum dyh*xhat", "rows", 0.5, t2.abs().sum(1), fam)
    s = s4.reshape(Gn, 4, C)
    a1 = act64(y, s[:, 2] if G > 1 else s4[2], s[:, 3] if G > 1 else s4[3], Gn)
    bound = torch.tensor(math.prod(sp) * float(a1.abs().max()))
    assert_exact(dW, wgrad_ref(dy.double(), a1), "dW", "f32", 0.5, bound, fam)
    return path


def _convt_case(c):
    sp, Cin, Cout = _shape(c), c["Cin"], c["Cout"]
    dims, seed, d = len(sp) - 1, c.get("seed", 5), c.get("dens", 0.5)
    x = tern(sp + (Cin,), d if not c.get("bn") else 0.6, seed)
    w = tern((Cin, Cout) + (2,) * dims, d, seed + 1).float()
    dout = tern((sp[0],) + tuple(2 * s for s in sp[1:]) + (Cout,), d, seed + 2)
    bn4 = bn_stats4(Cin, seed + 3) if c.get("bn") else None
    a = act64(x, bn4[2], bn4[3]) if bn4 is not None else x.double()
    q = 0.5 if bn4 is not None else 1.0
    return sp, dims, x, w, dout, bn4, a, q


def _convt_refs(a, w, dout, dims):
    fn = F.conv_transpose2d if dims == 2 else F.conv_transpose3d
    ar = cf(a).requires_grad_(True)
    wr = w.double().requires_grad_(True)
    out = fn(ar, wr, stride=2)
    gx, gw = torch.autograd.grad(out, [ar, wr], cf(dout))
    return cl(out.detach()), cl(gx), gw


def run_convt_fwd(o, dev, c):
    """convt_fwd with bias and the deferred BatchNorm of its input (bn4)."""
    sp, dims, x, w, dout, bn4, a, q = _convt_case(c)
    bias = int_bias(c["Cout"], c.get("seed", 5) + 4)
    out64, _, _ = _convt_refs(a, w, dout, dims)
    pk = pack(o, w, dev)
    out = o.convt_fwd(x.to(dev), pk.fwd, bias.to(dev), c["Cout"], None if bn4 is None else bn4.to(dev))
    path = o.last_path()
    assert_exact(out, out64 + bias.double(), "out", q=q, family="convt_fwd")
    return path


def run_convt_dgrad(o, dev, c):
    """convt_dgrad: dx and, with bn4, the BatchNorm-backward partial rows of the stored dx."""
    sp, dims, x, w, dout, bn4, a, q = _convt_case(c)
    _, gx, _ = _convt_refs(x.double(), w, dout, dims)
    pk = pack(o, w, dev)
    if bn4 is None:
        dx, part = o.convt_dgrad(dout.to(dev), pk.dgrad, c["Cin"])
    else:
        dx, part = o.convt_dgrad(dout.to(dev), pk.dgrad, c["Cin"], x.to(dev), bn4.to(dev))
    path = o.last_path()
    fam = "convt_dgrad"
    assert_exact(dx, gx, "dx", family=fam)
    if bn4 is not None:
        dyh, xh = bnb_terms(gx, x, bn4)
        rows = part.double().sum(0)
        s1, a1s = rows_ref(dyh)
        s2, a2s = rows_ref(dyh * xh)
        assert_exact(rows[0], s1, "BN rows sum dyh", "rows", 1.0, a1s, fam)
        assert_exact(rows[1], s2, "BN rows sum dyh*xhat", "rows", 0.5, a2s, fam)
    return path


def _assert_convt_grads(dW, db, gw, dout, a, q, fam):
    bound = torch.tensor(a[..., 0].numel() * float(a.abs().max()))
    assert_exact(dW.reshape(gw.shape), gw, "dW", "f32", q, bound, fam)
    s, sa = rows_ref(dout.double())
    assert_exact(db, s, "db", "f32", 1.0, sa, fam)


def run_convt_wgrad(o, dev, c):
    """convt_wgrad: dW and db, with the deferred BatchNorm of x (bn4)."""
    sp, dims, x, w, dout, bn4, a, q = _convt_case(c)
    _, _, gw = _convt_refs(a, w, dout, dims)
    dW, db = o.convt_wgrad(x.to(dev), dout.to(dev), None, None, None, None if bn4 is None else bn4.to(dev))
    path = o.last_path()
    _assert_convt_grads(dW, db, gw, dout, a, q, "convt_wgrad")
    return path


def run_convt_bwd_fused(o, dev, c):
    """convt_bwd_fused: everything the fused launch returns (dx, BN partial rows, dW, db)."""
    sp, dims, x, w, dout, bn4, a, q = _convt_case(c)
    _, gx, _ = _convt_refs(x.double(), w, dout, dims)
    _, _, gw = _convt_refs(a, w, dout, dims)
    pk = pack(o, w, dev)
    dx, part, dW, db = o.convt_bwd_fused(x.to(dev), dout.to(dev), pk.dgrad, None, None, None,
                                         None if bn4 is None else bn4.to(dev))
    path = o.last_path()
    fam = "convt_bwd_fused"
    assert_exact(dx, gx, "dx", family=fam)
    if bn4 is not None:
        dyh, xh = bnb_terms(gx, x, bn4)
        rows = part.double().sum(0)
        s1, a1s = rows_ref(dyh)
        s2, a2s = rows_ref(dyh * xh)
        assert_exact(rows[0], s1, "BN rows sum dyh", "rows", 1.0, a1s, fam)
        assert_exact(rows[1], s2, "BN rows sum dyh*xhat", "rows", 0.5, a2s, fam)
    else:
        assert part.numel() == 0
    _assert_convt_grads(dW, db, gw, dout, a, q, fam)
    return path


RUNNERS = {"fwd": run_conv3_fwd, "dgrad": run_conv3_dgrad, "wgrad": run_conv3_wgrad,
           "bwd32": run_conv3_bwd32, "convt_fwd": run_convt_fwd, "convt_dgrad": run_convt_dgrad,
           "convt_wgrad": run_convt_wgrad, "convt_bwd_fused": run_convt_bwd_fused}


def run_case(o, dev, kind, c):
    return RUNNERS[kind](o, dev, c)


# ------------------------------------------------------------------ non-linear kernels
def up2_ref(x64cf):
    mode = "bilinear" if x64cf.dim() == 4 else "trilinear"
    return F.interpolate(x64cf, scale_factor=2, mode=mode, align_corners=True)
