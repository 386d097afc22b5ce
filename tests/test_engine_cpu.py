"""The U-Net engine on the CPU: one code path, two kernel sets.

``UNetEngine`` calls ``torch.ops.ddlpc`` only; PyTorch dispatches each call to the gfx950
kernel (GPU tensors) or to the C++ reference kernel of ``csrc/cpu_ref.cpp`` (CPU tensors).
These tests run the whole engine — deferred BatchNorms, the two-pass head, the fused
32-channel backward, direct gradients into the flat buffer, the bucket reducer's readiness
triggers — on CPU tensors, against fp32 autograd through the stock modules, and train with
it through the ``Trainer`` (single process and a 2-rank gloo world).
"""
import statistics

import pytest
import torch
import torch.nn.functional as F

from dist_utils import run


def _model(dims, depth, mode, seed=0):
    from ddlpc.models import UNet
    torch.manual_seed(seed)
    return UNet(out_classes=6, depth=depth, dims=dims, up_sample_mode=mode).train()


def _grads(model, x, y, autocast=False):
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        loss, correct = model.loss_and_correct(x, y)
    loss.backward()
    return (float(loss), int(correct),
            [p.grad.detach().flatten().clone() if p.grad is not None else None
             for p in model.parameters()])


@pytest.mark.parametrize("dims,tile,depth,mode,B", [(2, 32, 5, "conv_transpose", 4),
                                                    (2, 32, 4, "bilinear", 4),
                                                    (3, 16, 3, "conv_transpose", 2)])
def test_engine_on_cpu_matches_fp32_autograd(dims, tile, depth, mode, B):
    """Loss, pixel accuracy, running statistics and every parameter gradient of one training
    step through the engine (bf16 activations, fp32 accumulation) against fp32 autograd on
    the same weights.  Gradient directions are held to the bf16 autocast run of the stock
    modules: per tensor at most 0.15 below it, the median at most 0.04 below it (at random
    init and this batch bf16 rounding alone moves deep-layer gradients by cos ~0.7-0.9)."""
    g = torch.Generator().manual_seed(7)
    x = torch.rand((B, 3) + (tile,) * dims, generator=g)
    y = torch.randint(0, 6, (B,) + (tile,) * dims, generator=g)
    ref = _model(dims, depth, mode)
    l0, c0, g0 = _grads(ref, x, y)
    ac = _model(dims, depth, mode)
    _, _, ga = _grads(ac, x, y, autocast=True)
    eng = _model(dims, depth, mode).to_hip()
    assert eng._engine is not None and eng._engine.side is None      # (no streams on a CPU)
    l1, c1, ge = _grads(eng, x, y)
    assert abs(l1 - l0) < 2e-3 * abs(l0)
    assert abs(c1 - c0) <= 0.01 * y.numel()
    for b0, b1 in zip(ref.buffers(), eng.buffers()):
        if b0.dtype.is_floating_point:
            assert torch.allclose(b0, b1, atol=5e-3, rtol=5e-3)
        else:
            assert torch.equal(b0, b1)
    cos_e, cos_a = [], []
    for (name, _), a, b, e in zip(ref.named_parameters(), g0, ga, ge):
        assert e is not None, name
        if name.endswith(".bias") and ("double_conv.0" in name or "double_conv.3" in name):
            assert torch.count_nonzero(e) == 0, name      # conv bias feeding a training BN
            continue
        ce, ca = float(F.cosine_similarity(a, e, dim=0)), float(F.cosine_similarity(a, b, dim=0))
        assert ce >= ca - 0.15, (name, ce, ca)
        cos_e.append(ce)
        cos_a.append(ca)
    assert statistics.median(cos_e) >= statistics.median(cos_a) - 0.04


def test_engine_cpu_inference_logits_match():
    """Eval-mode logits (running statistics, ``head_logits``) against the stock modules."""
    m = _model(2, 4, "conv_transpose")
    x = torch.rand(2, 3, 32, 32)
    ref = _model(2, 4, "conv_transpose")
    with torch.no_grad():
        for _ in range(2):                                   # move the running statistics
            ref(x)
        m.load_state_dict(ref.state_dict())
        m.eval(), ref.eval()
        l0 = ref(x)
        l1 = m.to_hip()(x)
    assert l1.shape == l0.shape
    assert float((l1 - l0).norm() / l0.norm()) < 3e-2


def test_synth_tiles_cpu_kernel_matches_host_twin():
    """The synthetic renderer's C++ kernel (the engine-layout batch on a CPU) and the PyTorch
    twin render the same bits; labels equal."""
    from ddlpc.data import SyntheticTiles
    for dims, tile in ((2, 48), (3, 12)):
        a = SyntheticTiles(9, tile, 6, 3, seed=3, dims=dims, layout="engine")
        b = SyntheticTiles(9, tile, 6, 3, seed=3, dims=dims, layout="nchw")
        idx = [0, 4, 8, 2]
        xa, ya = a.get(idx)
        xb, yb = b.get(idx)
        assert torch.equal(ya, yb)
        assert torch.equal(xa.float(), xb.bfloat16().float())


def _cfg(**kw):
    from ddlpc.config import ModelConfig, TrainConfig
    base = dict(model=ModelConfig(out_classes=6, depth=3), tile=32, num_samples=8,
                test_holdout=2, batch_per_gpu=2, accum_steps=1, epochs=1, log_every=0,
                log_dir=None, impl="hip", timeout_s=60)
    base.update(kw)
    return TrainConfig(**base)


def test_trainer_runs_the_engine_on_cpu(tmp_path):
    """``impl="hip"`` on a CPU: the Trainer attaches the engine (direct gradients into the
    flat buffer, the FlatAdam kernel), renders engine-layout batches with the synth_tiles
    CPU kernel, and trains; the loss falls over a few repeated steps."""
    from ddlpc.train.trainer import Trainer
    tr = Trainer(_cfg(ckpt_dir=str(tmp_path / "ck")), device="cpu")
    assert tr.impl == "hip" and tr.model._engine is not None and tr.model._engine.direct_grads
    x, y = tr.train_set.get([0, 1])
    assert getattr(x, "_ddlpc_nhwc", None) is not None      # the engine's padded layout
    losses = []
    for _ in range(6):
        tr.meter.reset()
        tr.train_step([(x, y)])
        losses.append(tr.meter.reduce()["loss"])
    assert all(l == l for l in losses) and losses[-1] < losses[0]
    tr.close()


def _engine_ranks(rank, world):
    from ddlpc.parallel import params_checksum
    from ddlpc.train.trainer import Trainer
    tr = Trainer(_cfg(check_consistency_every=1, bucket_mb=0.05), device="cpu")
    m = tr.fit()
    cs = float(params_checksum(tr.model))
    red = tr.reducer
    out = {"checksum": cs, "steps": tr.step_count, "loss": m["loss"],
           "buckets": len(red.buckets), "in_backward": red.stats["launched_in_backward"]}
    tr.close()
    return out


def test_engine_data_parallel_gloo_two_ranks():
    """Two CPU ranks training through the engine: the kernels' readiness calls trigger the
    bucket all-reduces during backward and the replicas stay bit-identical."""
    res = run(_engine_ranks, 2, ())
    assert res[0]["checksum"] == res[1]["checksum"]
    assert res[0]["steps"] == res[1]["steps"] > 0
    assert res[0]["buckets"] > 1 and res[0]["in_backward"] >= res[0]["buckets"]


@pytest.mark.gpu
@pytest.mark.parametrize("dims,tile,depth,mode,B", [(2, 64, 5, "conv_transpose", 4),
                                                    (2, 32, 4, "bilinear", 2),
                                                    (3, 16, 3, "conv_transpose", 2)])
def test_engine_cpu_kernels_match_gpu_kernels(dims, tile, depth, mode, B):
    """The same engine step on CPU tensors (csrc/cpu_ref.cpp) and on GPU tensors (the gfx950
    kernels): both follow one numerics contract (bf16 storage at the same points, fp32
    accumulation), so loss, accuracy, running statistics and gradients agree far more
    closely than either does with fp32."""
    g = torch.Generator().manual_seed(11)
    x = torch.rand((B, 3) + (tile,) * dims, generator=g)
    y = torch.randint(0, 6, (B,) + (tile,) * dims, generator=g)
    _, _, gref = _grads(_model(dims, depth, mode), x, y)          # fp32 stock modules
    cpu = _model(dims, depth, mode).to_hip()
    l0, c0, g0 = _grads(cpu, x, y)
    gpu = _model(dims, depth, mode).cuda().to_hip()
    l1, c1, g1 = _grads(gpu, x.cuda(), y.cuda())
    assert abs(l1 - l0) < 1e-3 * abs(l0)
    assert abs(c1 - c0) <= 0.002 * y.numel()
    for b0, b1 in zip(cpu.buffers(), gpu.buffers()):
        if b0.dtype.is_floating_point:
            assert torch.allclose(b0, b1.cpu(), atol=1e-3, rtol=1e-3)
    cos, cos32 = {}, {}
    for (name, _), a, b, r in zip(cpu.named_parameters(), g0, g1, gref):
        if float(a.norm()) == 0.0:
            assert float(b.norm()) == 0.0, name
            continue
        cos[name] = float(F.cosine_similarity(a, b.cpu(), dim=0))
        cos32[name] = float(F.cosine_similarity(r, b.cpu(), dim=0))
    # (fp32 summation order differs, so bf16 rounding flips at different elements; the deep
    # levels' tiny BN gradients carry the most of that.  Measured: per tensor >= 0.95, median
    # 0.98-0.995, where the GPU engine against fp32 has a median of ~0.9)
    worst = min(cos, key=cos.get)
    med, med32 = statistics.median(cos.values()), statistics.median(cos32.values())
    print("cos min", worst, cos[worst], "median", med, "| gpu vs fp32 median", med32)
    assert cos[worst] > 0.9, (worst, cos[worst])
    assert med > 0.97 and med > med32, (med, med32)


def test_bench_config1_engine_two_gloo_ranks():
    """BASELINE config #1 (4-level U-Net, 2 classes, CPU / gloo world 2) through the driver's
    launch line with the engine: the CPU kernels, direct gradients and bucketed gloo
    all-reduces; one JSON line, replicas bit-identical after the timed steps."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node", "2", "--rdzv-backend", "c10d",
                          "--rdzv-endpoint", "127.0.0.1:0", os.path.join(root, "bench.py"),
                          "--gpus", "2", "--impl", "hip", "--depth", "4", "--classes", "2",
                          "--tile", "64", "--batch", "2", "--steps", "2", "--warmup", "1",
                          "--bucket-mb", "0.5"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["impl"] == "hip" and rec["value"] > 0
    assert rec["dist_backend"] == "gloo" and rec["world_size"] == 2
    assert rec["replicas_identical"] is True and rec["config"]["buckets"] >= 2


def _window_step(bn_window):
    from ddlpc.train.trainer import Trainer
    torch.manual_seed(0)
    tr = Trainer(_cfg(batch_per_gpu=1, accum_steps=4, bn_window=bn_window, num_samples=8,
                      test_holdout=0), device="cpu")
    mbs = [tr.train_set.get([i]) for i in range(4)]
    grads, step = [], tr.optimizer.step

    def capture(*a, **k):                     # the accumulated gradient the optimizer sees
        grads.append(tr.flat.grad_buf.detach().clone())
        return step(*a, **k)
    tr.optimizer.step = capture
    tr.train_step(mbs)
    w = tr._window_size(4)
    g = grads[0]
    stats = torch.cat([b.detach().float().flatten() for b in tr.model.buffers()])
    tr.close()
    return w, g, stats


def test_bn_window_on_cpu_matches_micro_batches():
    """The reference regime (batch 1, accumulated micro-batches) as ONE batched pass with a
    BatchNorm statistics group per micro-batch (the BN-group kernels) equals running the
    micro-batches one by one, on the CPU kernels: the same accumulated gradient and running
    statistics up to bf16 rounding."""
    w1, g1, s1 = _window_step(-1)
    w0, g0, s0 = _window_step(0)
    assert w1 == 4 and w0 == 0
    # (measured: cosine 0.9993, relative L2 0.049 — bf16 rounding at different points)
    assert float(F.cosine_similarity(g1, g0, dim=0)) > 0.995
    assert float((g1 - g0).norm() / g0.norm()) < 0.1
    assert torch.allclose(s1, s0, rtol=1e-3, atol=1e-3)


def test_every_operator_has_cpu_and_gpu_kernels():
    """One op namespace, two kernels: every ``ddlpc::`` tensor operator registers a CUDA
    (gfx950) and a CPU kernel.  Exceptions: ``comm_proxy`` (a single-GPU stand-in for an RCCL
    collective) and the host-only planner settings and report (``set_cu_reserve``, ``set_knob``,
    ``last_path``)."""
    from ddlpc.ops import _ext
    _ext.load()
    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith("ddlpc::"))
    assert len(names) >= 40
    host_only = {"ddlpc::set_cu_reserve", "ddlpc::set_knob", "ddlpc::last_path"}
    for n in names:
        if n in host_only:
            continue
        assert torch._C._dispatch_has_kernel_for_dispatch_key(n, "CUDA"), n
        if n != "ddlpc::comm_proxy":
            assert torch._C._dispatch_has_kernel_for_dispatch_key(n, "CPU"), n
