"""The engine's schedule as an exact, device-independent trace (docs/TESTING.md, "Engine
schedule"): configurations, the tracer and the golden file, written once and run on both kernel
sets by ``test_engine_schedule_gpu.py`` and its ``test_engine_schedule_cpu.py`` twin.

``ddlpc/ops/fused_unet.py`` alone decides which operators a training step launches, in which
order, inside which weight-gradient stream segment, and when a parameter's gradient is reported
ready.  The engine tests hold its gradients to an fp32 oracle within bf16 tolerances, which a
dropped ``record_stream``, an early ``ready`` or a fall off a fused path all survive.  The trace
pins exactly those.

A trace of one step (``loss_and_correct`` + ``backward``, or an eval-mode forward) is the ordered
list of

* every ``torch.ops.ddlpc`` call of the engine, its arguments bound to the operator's schema (so
  positional and keyword passing, and an omitted argument and its default, read the same) and its
  results.  A tensor is written ``tN:dtype[shape]``; N numbers distinct tensors (storage, offset,
  sizes, strides) by first appearance, so the trace fingerprints the data flow and not only the
  operator names.  Every traced tensor is kept alive until the trace ends (no recycled pointers).
  Two things are a kernel's business and not the schedule's, and are left out so that both kernel
  sets give the same text: an empty placeholder tensor is written ``empty``, and the row count of
  a partial-sum slab (``ROW_RESULTS``: one row per workgroup of the producing grid) is ``*``;
* ``wgrad_stream`` segments: the enter with the non-empty tensors handed to it (the ones the GPU
  marks with ``record_stream`` and counts for the lag bound) and the exit.  Logged by a wrapper
  of the method when gradients are direct — otherwise, and on a CPU, the method hands out a null
  context; the wrapper logs before it delegates, so both devices give the same events;
* ``ready:<parameter name>`` for every ``grad_ready`` callback, and ``join`` for ``eng.join()``.

The tracer replaces the object ``fused_unet._ops()`` returns with a logging proxy: plain Python,
so it also sees the calls of the autograd engine's backward thread on a GPU.

``tests/golden/engine_schedule.json`` holds per configuration the readable event-name sequence,
the event count and the SHA-256 of the full trace text.  It was generated from the engine BEFORE
the orchestration was collapsed, and is regenerated only by a change that alters the schedule on
purpose:

    python tests/schedule_cases.py --write          # rewrite the golden file
    python tests/schedule_cases.py --dump DIR       # full traces as text (diff two checkouts)
    python tests/schedule_cases.py --digest         # SHA-256 of each run's gradients + buffers
"""
import contextlib
import hashlib
import json
import os
import sys
import threading

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_schedule.json")
CUS = 8                     # grids sized for 8 CUs (UNetEngine.c32_eligible depends on the count)
_DT = {torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64", torch.int64: "i64",
       torch.int32: "i32", torch.uint8: "u8", torch.bool: "b8", torch.float16: "f16"}


def ops():
    from ddlpc.ops import _ext
    return _ext.ops()


# ------------------------------------------------------------------ configurations
def case(name, tile=32, dims=2, batch=4, model=None, eng=None, loss=None, mode="train"):
    """model: UNet arguments over the base; eng: engine switches set by name; loss: "cw" (a
    class_weight vector) | "ignore" (ignore_index 255 on ~20 % of the labels); mode: "train"
    (run with returned and with direct gradients) | "eval" (model(x) under no_grad)."""
    return dict(name=name, tile=tile, dims=dims, batch=batch, model=model or {}, eng=eng or {},
                loss=loss, mode=mode)


SWITCHES = ["bwd32", "bnb_epilogue", "head_apply", "head_fused_fwd", "convt_fused",
            "wgrad_dy_prologue", "c32_bnp", "side_convt"]

CASES = [
    case("default"),
    *[case(f"{s}_off", eng={s: False}) for s in SWITCHES],
    case("defer_skip", eng=dict(defer_skip=True)),
    case("defer_mode_convt", eng=dict(defer_mode="convt")),
    case("defer_mode_none", eng=dict(defer_mode="none")),
    case("recompute1", eng=dict(recompute=1)),
    case("recompute2", eng=dict(recompute=2)),
    case("recompute1_defer_skip", eng=dict(recompute=1, defer_skip=True)),
    case("recompute2_defer_skip", eng=dict(recompute=2, defer_skip=True)),
    # tile 64: the 32-output-channel concat weight gradient is eligible at 8 CUs
    case("tile64", tile=64),
    case("tile64_c32_bnp_off", tile=64, eng=dict(c32_bnp=False)),
    case("bn_groups1", eng=dict(bn_groups=1)),
    case("bn_groups2_unfused", eng=dict(bn_groups=2, group_fuse_min_px=None)),
    case("bn_groups2_fused", eng=dict(bn_groups=2, group_fuse_min_px=64)),
    case("bilinear", model=dict(up_sample_mode="bilinear")),
    case("dims3", tile=16, dims=3, batch=2, model=dict(dims=3)),
    case("width_divisor1", model=dict(width_divisor=1)),
    case("class_weight", loss="cw"),
    case("ignore_index", loss="ignore"),
    case("eval", mode="eval"),
]
BY_NAME = {c["name"]: c for c in CASES}
TRAIN = [c["name"] for c in CASES if c["mode"] == "train"]
# the configurations a GPU runs (the trace is device-independent: same golden entries)
GPU_CASES = ["tile64", "bn_groups2_fused", "dims3"]
# switches whose two settings give identical gradients and buffers on the CPU kernels (on the
# GPU they select different kernels, so there the pairs are not comparable bit for bit)
IDENTICAL_PAIRS = [("default", "bwd32_off"), ("default", "convt_fused_off"),
                   ("default", "wgrad_dy_prologue_off"), ("default", "c32_bnp_off"),
                   ("tile64", "tile64_c32_bnp_off"), ("default", "side_convt_off"),
                   ("default", "defer_skip"), ("default", "recompute1"),
                   ("default", "recompute2"), ("defer_skip", "recompute1_defer_skip"),
                   ("defer_skip", "recompute2_defer_skip")]


def keys(names=None):
    """(case name, direct) of every run: both gradient modes for a training case"""
    out = []
    for n in (names or [c["name"] for c in CASES]):
        out += [(n, False), (n, True)] if BY_NAME[n]["mode"] == "train" else [(n, False)]
    return out


def key_id(name, direct):
    return name + ("-direct" if direct else "-returned") * (BY_NAME[name]["mode"] == "train")


# ------------------------------------------------------------------ the tracer
# Results that are slabs of per-workgroup partial sums ([rows][...], reduced by a later kernel):
# the row count is the producing kernel's grid, which differs between the kernel sets, so a slab's
# leading extent is written ``*``.  operator -> indices into its result list
ROW_RESULTS = {"conv3_fwd": (2,), "conv3_bwd32": (1,), "convt_dgrad": (1,), "convt_bwd_fused": (1,),
               "head_ce_fwd_stats": (1, 2), "head_ce_bwd": (3,)}


class Tracer:
    """Logging proxy for ``torch.ops.ddlpc`` (installed as ``fused_unet._F``) + the event list."""

    def __init__(self, real):
        self._real = real
        self.events, self.names = [], []
        self._ids, self._keep, self._fns = {}, [], {}
        self._lock = threading.Lock()

    def log(self, name, text):
        with self._lock:
            self.names.append(name)
            self.events.append(text)

    def label(self, t, rows=False):
        if t.numel() == 0:                       # (a placeholder: no storage, no data flow)
            return "empty"
        shape = tuple(t.shape)
        key = (t.untyped_storage().data_ptr(), t.storage_offset(), shape, t.stride(), t.dtype)
        with self._lock:
            ent = self._ids.get(key)
            if ent is None:
                ent = self._ids[key] = (len(self._ids), rows)
                self._keep.append(t)
        dims = ",".join(map(str, shape))
        if ent[1]:                               # (a kernel's grid, not the engine's schedule)
            dims = ",".join(["*"] + [str(d) for d in shape[1:]])
        return f"t{ent[0]}:{_DT.get(t.dtype, str(t.dtype))}[{dims}]"

    def fmt(self, v, rows=()):
        if isinstance(v, torch.Tensor):
            return self.label(v)
        if isinstance(v, (list, tuple)):
            return "[" + ", ".join(self.label(e, i in rows) if isinstance(e, torch.Tensor) else
                                   self.fmt(e) for i, e in enumerate(v)) + "]"
        return repr(v)

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            op = getattr(self._real, name)
            schema = op.default._schema.arguments

            def fn(*args, **kwargs):
                bound = {}
                for i, a in enumerate(schema):
                    if i < len(args):
                        assert a.name not in kwargs, (name, a.name)
                        bound[a.name] = args[i]
                    elif a.name in kwargs:
                        bound[a.name] = kwargs[a.name]
                    else:
                        assert a.has_default_value(), f"{name}: missing argument {a.name}"
                        bound[a.name] = a.default_value
                assert len(args) <= len(schema) and set(kwargs) <= {a.name for a in schema}, name
                head = f"{name}(" + ", ".join(f"{k}={self.fmt(v)}" for k, v in bound.items()) + ")"
                out = op(*args, **kwargs)
                self.log(name, head + " -> " + self.fmt(out, ROW_RESULTS.get(name, ())))
                return out
            self._fns[name] = fn
        return fn

    def text(self):
        return "\n".join(self.events) + "\n"


class _Segment:
    def __init__(self, tracer, ctx):
        self.tracer, self.ctx = tracer, ctx

    def __enter__(self):
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self.tracer.log("}", "wgrad_stream exit")
        return self.ctx.__exit__(*exc)


@contextlib.contextmanager
def tracing(model, ready_names):
    """Trace the engine of ``model`` inside the block: -> the Tracer."""
    from ddlpc.ops import fused_unet as fu
    eng = model._engine
    tr = Tracer(ops())
    real_ws, real_join = eng.wgrad_stream, eng.join

    def wgrad_stream(*tensors):
        if not eng.direct_grads:                 # (no segment: the method's null context)
            return real_ws(*tensors)
        marked = [tr.label(t) for t in tensors if isinstance(t, torch.Tensor) and t.numel()]
        tr.log("stream{", "wgrad_stream enter [" + ", ".join(marked) + "]")
        return _Segment(tr, real_ws(*tensors))

    def join():
        tr.log("join", "join")
        return real_join()

    def grad_ready(p):
        tr.log("ready:" + ready_names[id(p)], "ready:" + ready_names[id(p)])

    prev = fu._F
    fu._F = tr
    eng.wgrad_stream, eng.join = wgrad_stream, join
    if eng.direct_grads:
        eng.grad_ready = grad_ready
    try:
        yield tr
    finally:
        fu._F = prev
        del eng.wgrad_stream, eng.join
        if eng.direct_grads:
            eng.grad_ready = None


# ------------------------------------------------------------------ one run
class Result:
    def __init__(self, tracer, tensors):
        self.names = tracer.names
        self.count = len(tracer.events)
        self.text = tracer.text()
        self.sha256 = hashlib.sha256(self.text.encode()).hexdigest()
        self.tensors = tensors                   # name -> CPU tensor (loss, grads, buffers)

    def digest(self):
        h = hashlib.sha256()
        for k, v in self.tensors.items():
            h.update(k.encode())
            h.update(v.reshape(-1).view(torch.uint8).numpy().tobytes())
        return h.hexdigest()


@contextlib.contextmanager
def eight_cus():
    o = ops()
    before = int(o.set_cu_reserve(-1))
    phys = int(o.set_cu_reserve(0))
    o.set_cu_reserve(phys - CUS)
    assert int(o.set_cu_reserve(-1)) == CUS
    try:
        yield
    finally:
        o.set_cu_reserve(phys - before)


_RUNS = {}


def run(name, direct, dev="cpu"):
    """One traced step of configuration ``name`` (cached: the tests share the runs)."""
    k = (name, bool(direct), dev)
    if k not in _RUNS:
        with eight_cus():
            _RUNS[k] = _run(BY_NAME[name], bool(direct), dev)
    return _RUNS[k]


def _run(c, direct, dev):
    from ddlpc.models import UNet
    torch.manual_seed(0)
    margs = dict(out_classes=6, depth=3, width_divisor=2)
    margs.update(c["model"])
    model = UNet(**margs).train().to(dev).to_hip()
    eng = model._engine
    for k, v in c["eng"].items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    g = torch.Generator().manual_seed(7)
    sp = (c["tile"],) * c["dims"]
    x = torch.rand((c["batch"], 3) + sp, generator=g).to(dev)
    y = torch.randint(0, 6, (c["batch"],) + sp, generator=g)
    kw = {}
    if c["loss"] == "ignore":
        y[torch.rand(y.shape, generator=g) < 0.2] = 255
        kw["ignore_index"] = 255
    elif c["loss"] == "cw":
        kw["class_weight"] = torch.tensor([0.3, 0.0, 3.0, 0.7, 1.9, 1.0], device=dev)
    y = y.to(dev)
    names = {id(p): n for n, p in model.named_parameters()}
    out = {}
    if c["mode"] == "eval":
        model.eval()
        with tracing(model, names) as tr, torch.no_grad():
            out["logits"] = model(x)
    else:
        if direct:
            for p in model.parameters():
                p.grad = torch.zeros_like(p)
            eng.enable_direct_grads(None)
        with tracing(model, names) as tr:
            loss, correct = model.loss_and_correct(x, y, **kw)
            loss.backward()
        out["loss"], out["correct"] = loss.detach(), correct
        for n, p in model.named_parameters():
            assert p.grad is not None, n
            out["grad:" + n] = p.grad
    for n, b in model.named_buffers():
        out["buffer:" + n] = b
    if dev != "cpu":
        torch.cuda.synchronize()
    return Result(tr, {k: v.detach().cpu().clone() for k, v in out.items()})


def same_results(a, b):
    """-> names of the tensors (loss, gradients, buffers) that differ between two runs"""
    assert a.tensors.keys() == b.tensors.keys()
    return [k for k in a.tensors if not torch.equal(a.tensors[k], b.tensors[k])]


# ------------------------------------------------------------------ the golden file
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _write(path):
    lines = []
    for name, direct in keys():
        r = run(name, direct)
        rows, row = [], "   "
        for n in r.names:
            if len(row) + len(n) + 4 > 100:
                rows.append(row)
                row = "   "
            row += f' "{n}",'
        rows.append(row)
        body = "\n".join(rows).rstrip(",")
        lines.append(f' "{key_id(name, direct)}": {{"count": {r.count}, "sha256": "{r.sha256}",\n'
                     f'  "events": [\n{body}]}}')
    text = "{\n" + ",\n".join(lines) + "\n}\n"
    json.loads(text)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", action="store_true", help="regenerate tests/golden/engine_schedule.json")
    ap.add_argument("--dump", metavar="DIR", help="write every configuration's full trace as text")
    ap.add_argument("--digest", action="store_true",
                    help="print the SHA-256 of every run's loss, gradients and buffers")
    ap.add_argument("--device", default="cpu")
    args = ap.parse_args(argv)
    if args.write:
        assert args.device == "cpu"
        _write(GOLDEN)
        print("wrote", GOLDEN)
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        for name, direct in keys():
            with open(os.path.join(args.dump, key_id(name, direct) + ".txt"), "w") as f:
                f.write(run(name, direct, args.device).text)
    if args.digest:
        for name, direct in keys():
            print(key_id(name, direct), run(name, direct, args.device).digest())


if __name__ == "__main__":
    main(sys.argv[1:])
