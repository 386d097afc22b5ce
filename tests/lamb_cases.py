"""Cases for ``lamb_step`` (``csrc/lamb.hip``, CPU twin in ``csrc/cpu_ref.cpp``, arithmetic in
``csrc/lamb_math.h``), run on both kernel sets by ``test_lamb_gpu.py`` and ``test_lamb_cpu.py``.

Each step is checked on its own: the kernels' fp32 ``p, m, v`` before the call and the device's own
scalar table go into an fp64 evaluation of the documented expression.  u = 2^-24; every fp32
operation rounds once (no contraction); second-order terms: ``adam_ref``'s factor 1 + 2^-10.

    m', v'            ``sched_ref`` (``adam_ref`` with gc = g coef, no decay): Em, Ev
    s = sqrt(v')      Es = Ev / (sqrt(v') + sqrt(max(v' - Ev, 0))) + u s               (as adam_ref)
    d = s isb2 + eps  Ed = isb2 Es + u s isb2 + u d
    r = (m' ibc1) / d Er = (ibc1 Em + u |m' ibc1| + |r| Ed) / (d - Ed) + u |r|         (adam_ref's Eq)
    u_ = r + wd p     Eu = Er + u |wd p| + u |u_|              (excluded tensor or wd = 0: Eu = Er)
    ||p||             exact fp32 inputs, fp64 sums (relative error n 2^-53, far below u), one fp32
                      cast: E = u ||p||
    ||u_||            the kernel sums its own fp32 u_: | ||u_dev|| - ||u_ref|| | <= ||Eu||_2 (triangle
                      inequality), then the cast: E = ||Eu||_2 + u (||u_ref|| + ||Eu||_2)
    ratio             ||p|| / ||u_|| in double from the double norms, one fp32 cast:
                      E = ratio ||Eu||_2 / (||u_ref|| - ||Eu||_2) + u ratio; exactly 1 for an excluded
                      tensor and where a norm is 0
    p' = p - step u_  step = fl(lr_t ratio) of the device's fp32 lr_t and ratio (exact in double, so
                      the reference forms the kernel's step itself): Ep = |step| Eu + u |step u_| + u |p'|
"""
import math

import torch

from sched_cases import sched_ref
from update_cases import ADAM, SENT, U, _gen, adam_grad, assert_bits, f32, ops, record, ulp32  # noqa: F401

K = 1 + 2.0 ** -10
GAP_G = 1e30                  # the gradient's gaps: finite, but its square overflows fp32
# "vec" is the 1-D tensor (excluded under exclude_1d), "pzero" has p = 0, "gzero" g = 0; "strided"
# has 301 chunks: more than the ratio kernel's 256 threads
LAYOUT = [("a1", 1), ("a3", 3), ("a64", 64), ("a1023", 1023), ("a1024", 1024), ("a1025", 1025),
          ("three", 2 * 1024 + 5), ("strided", 300 * 1024 + 7), ("vec", 100), ("pzero", 1030), ("gzero", 1500)]
NCHUNKS = 316
SCHED = (1, 2, 10, 1e-5, 0.9)      # poly, warm-up 2 of 10 steps, lr_min, power


class State:
    """p, g, m, v over LAYOUT's 64-aligned spans with sentinel gaps, and the operator's buffers"""

    def __init__(self, dev, exclude_1d=True, seed=21):
        from ddlpc.ops.lamb import lamb_tables
        self.span, o = {}, 64                       # (a gap in front of the first tensor too)
        for name, n in LAYOUT:
            self.span[name] = (o, o + n)
            o += (n + 63) // 64 * 64
        self.n = o + 64
        self.adapted = [not (exclude_1d and name == "vec") for name, _ in LAYOUT]
        chunks, tensors = lamb_tables(list(self.span.values()), self.adapted)
        assert int(tensors[7, 1]) == 301 and chunks.shape[0] == NCHUNKS
        self.inside = torch.zeros(self.n, dtype=torch.bool)
        for a, b in self.span.values():
            self.inside[a:b] = True
        p = torch.where(self.inside, torch.randn(self.n, generator=_gen(seed)), torch.tensor(SENT))
        p[slice(*self.span["pzero"])] = 0.0
        mv = torch.where(self.inside, torch.tensor(0.0), torch.tensor(SENT))
        self.p, self.m, self.v, self.g = p.to(dev), mv.to(dev), mv.clone().to(dev), torch.full((self.n,), GAP_G).to(dev)
        self.chunks, self.tensors = chunks.to(dev), tensors.to(dev)
        self.scal = torch.zeros(8, device=dev)
        self.partial = torch.zeros(3 * NCHUNKS, dtype=torch.float64, device=dev)
        self.ratio, self.norms = torch.zeros(len(LAYOUT), device=dev), torch.zeros(len(LAYOUT), 2, device=dev)

    def grad(self, t, seed=21):
        g = torch.where(self.inside, adam_grad(self.n, t, seed), torch.tensor(GAP_G))
        g[slice(*self.span["gzero"])] = 0.0
        self.g.copy_(g)
        return g

    def call(self, o, wd=0.0, max_norm=0.0, **over):
        a = dict(p=self.p, g=self.g, m=self.m, v=self.v, scal=self.scal, chunks=self.chunks, tensors=self.tensors,
                 partial=self.partial, ratio=self.ratio, norms=self.norms)
        a.update(over)
        o.lamb_step(*a.values(), ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], wd, max_norm, *SCHED)


def lamb_ref(p0, m0, v0, g, wdt, ibc1, isb2, coef):
    """-> (m', Em), (v', Ev), (u_, Eu) of one tensor (the docstring's derivation; wdt = 0: u_ = r)"""
    b1, b2, eps = f32(ADAM["b1"]), f32(ADAM["b2"]), f32(ADAM["eps"])
    (mr, Em), (vr, Ev), _ = sched_ref(p0, m0, v0, g, b1, b2, eps, 0.0, ibc1, isb2, coef, 0.0, False)
    s = vr.sqrt()
    lo = s + (vr - Ev).clamp_min(0.0).sqrt()
    Es = torch.where(lo > 0, Ev / lo.clamp_min(1e-300), torch.zeros_like(Ev)) + U * s
    d = s * isb2 + eps
    Ed = isb2 * Es + U * s * isb2 + U * d
    assert bool((d - Ed > 0).all()), "bad case: the denominator is not bounded away from zero"
    num = ibc1 * mr
    r = num / d
    Er = (ibc1 * Em + U * num.abs() + r.abs() * Ed) / (d - Ed) + U * r.abs()
    if wdt == 0.0:
        return (mr, Em), (vr, Ev), (r, K * Er)
    u = r + wdt * p0.double()
    return (mr, Em), (vr, Ev), (u, K * (Er + U * (wdt * p0.double()).abs() + U * u.abs()))


def run_stages(o, dev, wd, clip, exclude_1d, steps=3):
    from ddlpc.ops.adam import schedule_lr
    st = State(dev, exclude_1d)
    max_norm = 0.05 * math.sqrt(int(st.inside.sum())) if clip else 0.0      # (adam_grad's norm: 0.19 sqrt(n))
    fam = f"lamb_step{' clip' if clip else ''}{' wd' if wd else ''}"
    for t in range(1, steps + 1):
        g = st.grad(t)
        p0, m0, v0 = st.p.cpu().clone(), st.m.cpu().clone(), st.v.cpu().clone()
        st.call(o, wd=wd, max_norm=max_norm)
        sc = [float(x) for x in st.scal.cpu()]
        p1, m1, v1, ratio, norms = st.p.cpu(), st.m.cpu(), st.v.cpu(), st.ratio.cpu().double(), st.norms.cpu().double()
        # the scalar table against the Python doubles (the gradient norm: the tensors', not the gaps')
        gn = math.sqrt(math.fsum((g[st.inside].double() ** 2).tolist())) if clip else 0.0
        want = [float(t), 1 / (1 - ADAM["b1"] ** t), 1 / math.sqrt(1 - ADAM["b2"] ** t),
                schedule_lr(t, ADAM["lr"], "poly", *SCHED[1:]), gn, min(max_norm / (gn + 1e-6), 1.0) if clip else 1.0,
                0.0, 0.0]
        for i, (got, w) in enumerate(zip(sc, want)):
            assert abs(got - w) <= (ulp32(w) if w else 0.0), (i, t, got, w)
        assert (sc[5] < 1.0) == clip, "bad case: max_norm does not clip"
        for k, (name, _) in enumerate(LAYOUT):
            a, b = st.span[name]
            wdt = f32(wd) if st.adapted[k] else 0.0
            (mr, Em), (vr, Ev), (u, Eu) = lamb_ref(p0[a:b], m0[a:b], v0[a:b], g[a:b], wdt, sc[1], sc[2], sc[5])
            record(fam + " m", m1[a:b], mr, Em)
            record(fam + " v", v1[a:b], vr, Ev)
            npr, nur, EuN = float(p0[a:b].double().norm()), float(u.norm()), float(Eu.norm())
            one = not st.adapted[k] or npr == 0.0 or nur == 0.0
            rr = 1.0 if one else npr / nur
            assert one or nur > 2 * EuN, "bad case: ||u|| is not bounded away from zero"
            Er = 0.0 if one else K * (rr * EuN / (nur - EuN) + U * rr)
            record(fam + " ratio", ratio[k:k + 1], torch.tensor([rr]), torch.tensor([Er]))
            record(fam + " norms", norms[k], torch.tensor([npr, nur]), K * torch.tensor([U * npr, EuN + U * (nur + EuN)]))
            step = f32(sc[3] * float(ratio[k]))
            pr = p0[a:b].double() - step * u
            record(fam + " p", p1[a:b], pr, K * (abs(step) * Eu + U * (step * u).abs() + U * pr.abs()))
            if name == "pzero" and t == 1:
                assert float(ratio[k]) == 1.0 and npr == 0.0
            if name == "gzero" and wdt == 0.0:
                assert float(ratio[k]) == 1.0 and nur == 0.0
                assert_bits(p1[a:b], p0[a:b], "p where u = 0")
        for name, x in (("p", p1), ("m", m1), ("v", v1)):
            assert bool((x[~st.inside] == SENT).all()), f"{name}: a gap was written at step {t}"
        assert torch.equal(st.g.cpu(), g), "the gradient was written"


def run_capture():
    """two copies of one state: the same bits after a step each, then 3 replays of a captured step() against 3 eager"""
    from ddlpc.ops.lamb import FlatLamb
    from ddlpc.parallel.flat import FlatParams
    opts = []
    for _ in range(2):                               # the eager optimizer, the captured one
        torch.manual_seed(3)
        flat = FlatParams([torch.nn.Parameter(torch.randn(s, device="cuda")) for s in ((37, 29, 3), (37,), (5000,), (2, 3))])
        flat.grad_buf.copy_(torch.randn(flat.numel, generator=_gen(5)).to("cuda"))
        opts.append(FlatLamb(flat, weight_decay=0.01, max_grad_norm=1.0, lr_schedule="cosine", warmup_steps=6,
                             total_steps=8, lr_min=1e-5))    # (steps 2..4 are on the warm-up's ramp)
        opts[-1].step()                         # (the table's check on the host; both take it)
    (eager, cap), graph, lrs = opts, torch.cuda.CUDAGraph(), []
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        cap.step()
    for t in range(1, 5):
        if t > 1:
            eager.step()
            graph.replay()
        for name in ("exp_avg", "exp_avg_sq", "ratio", "_dev_scal"):
            assert_bits(getattr(cap, name), getattr(eager, name), f"{name} at step {t}")
        assert_bits(cap.flat.param_buf, eager.flat.param_buf, f"p at step {t}")
        s = cap.last_stats()
        assert float(cap._dev_scal[0]) == t and abs(s["lr"] - cap.lr_at(t)) <= ulp32(cap.lr_at(t))
        assert 0 < s["trust_min"] <= s["trust_max"] and s["clip_coef"] < 1.0
        lrs.append(s["lr"])
    assert len(set(lrs)) == 4, "the learning rate did not advance through the replays"


def _patched(st, row, col, val):
    d = st.chunks.device
    return st.chunks.index_put((torch.tensor(row, device=d), torch.tensor(col, device=d)), torch.tensor(val, device=d))


# name -> (argument, its bad value for a State): calls that both registrations must refuse before touching memory
REFUSALS = {
    "p fp64": ("p", lambda st: st.p.double()),
    "m on the host": ("m", lambda st: st.m.cpu()),          # (GPU only)
    "m strided": ("m", lambda st: torch.zeros(2 * st.n, device=st.p.device)[::2]),
    "ratio shorter than the tensors": ("ratio", lambda st: st.ratio[:-1]),
    "chunk past the buffer": ("chunks", lambda st: _patched(st, NCHUNKS - 1, 1, st.n - 64)),
    "chunk into the next tensor": ("chunks", lambda st: _patched(st, 2, 2, 128)),
    "chunk off its tensor's pieces": ("chunks", lambda st: _patched(st, 8, 1, int(st.chunks[8, 1]) + 1024)),
}


def run_refusal(o, dev, name):
    st = State(dev)
    st.grad(1)
    st.call(o, **{REFUSALS[name][0]: REFUSALS[name][1](st)})
