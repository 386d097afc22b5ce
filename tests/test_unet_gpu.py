"""End-to-end U-Net on the HIP kernels vs the stock-PyTorch fp32 oracle (same weights)."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"      # (tests/test_unet_cpu.py re-runs a subset with DEV = "cpu": the CPU kernels)


def _sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-30))


@pytest.mark.parametrize("depth,wd,tile,mode,dims,classes", [
    (5, 2, 128, "conv_transpose", 2, 6), (4, 4, 64, "bilinear", 2, 6),
    (3, 4, 32, "conv_transpose", 3, 6),
    (5, 1, 64, "conv_transpose", 2, 6),      # standard U-Net widths (NN_in_model = 1, ref.py:687)
    (4, 2, 64, "conv_transpose", 2, 3),      # out_classes 3 (the CPU DP tests' config)
    (4, 4, 64, "bilinear", 2, 11)])          # 16-channel head, 11 classes (padded to 16)
def test_unet_engine_matches_torch(depth, wd, tile, mode, dims, classes):
    """HIP bf16 gradients must be as close to the fp32 oracle as stock PyTorch bf16 autocast."""
    from ddlpc.models import UNet
    torch.manual_seed(0)
    ref = UNet(out_classes=classes, width_divisor=wd, depth=depth, up_sample_mode=mode,
               dims=dims).to(DEV)
    amp = copy.deepcopy(ref)
    hip = copy.deepcopy(ref).to_hip()
    N = 4
    shape = (N, 3) + (tile,) * dims
    x = torch.rand(shape, device=DEV).bfloat16().float()
    y = torch.randint(0, classes, (N,) + (tile,) * dims, device=DEV)
    loss_r = F.cross_entropy(ref(x), y)
    loss_r.backward()
    with torch.autocast(DEV, dtype=torch.bfloat16):
        loss_a = F.cross_entropy(amp(x).float(), y)
    loss_a.backward()
    loss_h, correct = hip.loss_and_correct(x, y)
    loss_h.backward()
    assert abs(float(loss_h) - float(loss_r)) < 2e-2 * float(loss_r)
    worst = []
    for (n, pr), (_, pa), (_, ph) in zip(ref.named_parameters(), amp.named_parameters(),
                                          hip.named_parameters()):
        if n.endswith((".0.bias", ".3.bias")) and "double_conv.double_conv" in n:
            assert float(ph.grad.abs().max()) == 0.0      # BN-cancelled conv bias
            continue
        ch, ca = _cos(pr.grad, ph.grad), _cos(pr.grad, pa.grad)
        worst.append((ch - ca, n, ch, ca))
        assert ch > min(0.98, ca - 0.08), (n, ch, ca)
    print("worst hip-vs-amp cosine deltas:", sorted(worst)[:4])
    med_h = sorted(w[2] for w in worst)[len(worst) // 2]
    med_a = sorted(w[3] for w in worst)[len(worst) // 2]
    assert med_h > med_a - 0.02, (med_h, med_a)
    # running statistics updated like nn.BatchNorm
    for (n, br), (_, bh) in zip(ref.named_buffers(), hip.named_buffers()):
        if "running" in n:
            assert torch.allclose(br, bh, rtol=2e-2, atol=2e-2), n
    # eval-mode logits
    ref.eval(), hip.eval()
    with torch.no_grad():
        lr, lh = ref(x), hip(x)
    assert _cos(lr, lh) > 0.99


def test_unet_engine_flagship_gradients_tight():
    """The flagship geometry (depth 5, width/2, 6 classes, transposed-conv up-sampling) at 128²
    batch 4 against the fp32 oracle, with stock bf16 autocast as the yardstick of what bf16
    arithmetic can reach on each tensor:

    * every gradient tensor on which autocast reaches cosine >= 0.995: the HIP engine >= 0.99
      (absolute), the head >= 0.999;
    * the rest — the deep layers, whose train-mode BatchNorms normalise 2x2 .. 8x8 pixels x 4
      images and amplify any bf16 rounding (autocast itself: cosine 0.8-0.95 there) — within
      0.03 of autocast, and the median over all tensors within 0.005 of autocast's;
    * running statistics: running_var within rtol 5e-3, running_mean within 5e-3 of
      (|mean| + running std)."""
    from ddlpc.models import UNet
    torch.manual_seed(0)
    ref = UNet(out_classes=6).to(DEV)
    amp = copy.deepcopy(ref)
    hip = copy.deepcopy(ref).to_hip()
    x = torch.rand(4, 3, 128, 128, device=DEV).bfloat16().float()
    y = torch.randint(0, 6, (4, 128, 128), device=DEV)
    F.cross_entropy(ref(x), y).backward()
    with torch.autocast(DEV, dtype=torch.bfloat16):
        loss_a = F.cross_entropy(amp(x).float(), y)
    loss_a.backward()
    loss_h, _ = hip.loss_and_correct(x, y)
    loss_h.backward()
    bad, rows = [], []
    for (n, pr), (_, pa), (_, ph) in zip(ref.named_parameters(), amp.named_parameters(),
                                          hip.named_parameters()):
        if n.endswith((".0.bias", ".3.bias")) and "double_conv.double_conv" in n:
            continue                                  # BN-cancelled conv bias (exact zero)
        ch, ca = _cos(pr.grad, ph.grad), _cos(pr.grad, pa.grad)
        rows.append((round(ch, 4), round(ca, 4), n))
        if ca >= 0.995:
            ok = ch >= (0.999 if n.startswith("conv_last") else 0.99)
        else:
            ok = ch >= ca - 0.03
        if not ok:
            bad.append((n, ch, ca))
    print("gradient cosines (hip, autocast), lowest 8:", sorted(rows)[:8])
    print("tensors held to the absolute 0.99:", sum(1 for r in rows if r[1] >= 0.995), "of", len(rows))
    assert not bad, bad
    med_h = sorted(r[0] for r in rows)[len(rows) // 2]
    med_a = sorted(r[1] for r in rows)[len(rows) // 2]
    assert med_h >= med_a - 0.005, (med_h, med_a)
    bufs = dict(ref.named_buffers())
    for n, bh in hip.named_buffers():
        if "running_mean" in n:
            br = bufs[n]
            std = bufs[n.replace("running_mean", "running_var")].sqrt()
            assert torch.all((bh - br).abs() <= 5e-3 * (br.abs() + std)), n
        elif "running_var" in n:
            assert torch.allclose(bh, bufs[n], rtol=5e-3, atol=0), n


def test_trainer_hip_step_decreases_loss():
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=4,
                      num_samples=1, test_holdout=0, impl="hip")
    tr = Trainer(cfg, device=DEV)
    x, y = device_random_batch(4, 64, 6, tr.device)
    losses = []
    for _ in range(8):
        tr.train_step([(x, y)])
        losses.append(tr.meter.reduce()["loss"])
        tr.meter.reset()
    assert losses[-1] < losses[0]
    tr.close()


def test_trainer_hip_graph_matches_eager():
    """cfg.hip_graph: the captured/replayed step reproduces the eager step (same kernels,
    device-side Adam bias corrections) — parameters, optimizer state and metrics."""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    batches = None
    out = []
    for graph in (False, True):
        cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=4,
                          num_samples=1, test_holdout=0, impl="hip", hip_graph=graph)
        tr = Trainer(cfg, device=DEV)
        if batches is None:
            batches = [device_random_batch(4, 64, 6, tr.device, seed=s) for s in range(3)]
        losses = []
        for i in range(7):                       # 3 eager warm-up + capture, then replays
            tr.train_step([batches[i % 3]])
            losses.append(tr.meter.reduce()["loss"])
            tr.meter.reset()
        if graph:
            assert "last" in tr._graphs, "step was not captured"
        assert tr.optimizer.step_count == 7 and tr.step_count == 7
        out.append((tr.flat.param_buf.clone(), tr.optimizer.exp_avg_sq.clone(), losses))
        tr.close()
    (p0, v0, l0), (p1, v1, l1) = out
    # every kernel is deterministic (no float atomics on this path), so replay == eager
    assert torch.equal(p0, p1), float((p0 - p1).abs().max())
    assert torch.equal(v0, v1)
    assert l0 == l1


@pytest.mark.parametrize("accum", [3])
def test_trainer_hip_graph_accumulation_matches_eager(accum):
    """cfg.hip_graph with accumulation (the reference's regime: many micro-batches per
    optimizer step, ref.py:685,750-766): the "acc" graph replays every non-final micro-batch
    and the "last" graph the final micro-batch + Adam.  Parameters, Adam moments, BN running
    statistics and per-step losses are bit-identical to the eager schedule."""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    out = []
    for graph in (False, True):
        cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=1,
                          num_samples=1, test_holdout=0, impl="hip", hip_graph=graph,
                          accum_steps=accum, micro_streams=1, bn_window=0)
        tr = Trainer(cfg, device=DEV)
        tr.model._engine.set_side_stream(False)
        batches = [device_random_batch(1, 64, 6, tr.device, seed=s) for s in range(5)]
        losses = []
        for i in range(5):                       # 3 eager warm-ups per graph kind, then replays
            tr.train_step([batches[(i + j) % 5] for j in range(accum)])
            losses.append(tr.meter.reduce()["loss"])
            tr.meter.reset()
        if graph:
            assert set(tr._graphs) == {"acc", "last"}, tr._graphs.keys()
        assert tr.optimizer.step_count == 5 and tr.step_count == 5
        assert tr.micro_count == 5 * accum
        _sync()
        out.append((tr.flat.param_buf.clone(), tr.optimizer.exp_avg_sq.clone(), losses,
                    {k: v.clone() for k, v in tr.model.state_dict().items() if "running" in k}))
        tr.close()
    (p0, v0, l0, b0), (p1, v1, l1, b1) = out
    assert torch.equal(p0, p1), float((p0 - p1).abs().max())
    assert torch.equal(v0, v1)
    assert l0 == l1
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k


def _short_batch_run(graph, accum, steps):
    """``steps``: per train_step call, the batch sizes of its micro-batches.  Every micro-batch
    is its own seeded batch.  -> parameters, second moments, running statistics, step losses."""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=4, num_samples=1,
                      test_holdout=0, impl="hip", hip_graph=graph, accum_steps=accum,
                      micro_streams=1, bn_window=0)
    tr = Trainer(cfg, device=DEV)
    tr.model._engine.set_side_stream(False)
    losses, seed = [], 0
    for sizes in steps:
        mbs = []
        for b in sizes:
            mbs.append(device_random_batch(b, 64, 6, tr.device, seed=seed))
            seed += 1
        tr.train_step(mbs)
        losses.append(tr.meter.reduce()["loss"])
        tr.meter.reset()
    assert tr.optimizer.step_count == tr.step_count == len(steps)
    assert tr.micro_count == sum(len(s) for s in steps)
    if graph:
        assert set(tr._graphs) == ({"last"} if accum == 1 else {"acc", "last"})
    _sync()
    out = (tr.flat.param_buf.clone(), tr.optimizer.exp_avg_sq.clone(),
           {k: v.clone() for k, v in tr.model.state_dict().items() if "running" in k}, losses)
    tr.close()
    return out


def _assert_runs_equal(eager, graph):
    (p0, v0, b0, l0), (p1, v1, b1, l1) = eager, graph
    assert torch.equal(p0, p1), float((p0 - p1).abs().max())
    assert torch.equal(v0, v1)
    assert l0 == l1, (l0, l1)
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k


def test_hip_graph_short_batch_matches_eager():
    """A short batch (``ShardedSampler.batches`` without drop_last ends an epoch on one) replaces
    the graphs' static inputs, so the "last" graph captured over the old ones is dropped and
    warms up again: calls 1-5 run a batch of 4 (the fifth replays), call 6 a batch of 2, calls
    7-9 batches of 4 (re-captured on call 9).  Bit-identical to the eager schedule: every kernel
    on this path is deterministic."""
    steps = [[4]] * 5 + [[2]] + [[4]] * 3
    _assert_runs_equal(_short_batch_run(False, 1, steps), _short_batch_run(True, 1, steps))


def test_hip_graph_short_micro_batch_in_window_matches_eager():
    """The same with accumulation: the short micro-batch sits in the middle of one window, so
    the "acc" graph stages it and both graphs lose the static inputs they share.  Parameters,
    moments, running statistics and losses equal the eager schedule's."""
    steps = [[4, 4, 4]] * 5 + [[4, 2, 4]] + [[4, 4, 4]] * 3
    _assert_runs_equal(_short_batch_run(False, 3, steps), _short_batch_run(True, 3, steps))


def test_phase_marks_per_schedule():
    """The phase marks of a step, by schedule (``PhaseTimer.read()`` stays comparable with
    recorded runs): eager start / fwd_bwd / optimizer; single-GPU graph start only, since
    the optimizer runs inside the "last" graph.  (With a reducer: tests/test_trainer.py.)"""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    for graph, want in ((False, {"fwd_bwd_ms", "optimizer_ms", "step_ms"}), (True, {"step_ms"})):
        cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=2, num_samples=1,
                          test_holdout=0, impl="hip", hip_graph=graph, phase_timers=True)
        tr = Trainer(cfg, device=DEV)
        batch = device_random_batch(2, 64, 6, tr.device)
        for _ in range(5):                       # the fifth is a replay
            tr.train_step([batch])
        _sync()
        assert ("last" in tr._graphs) == graph
        assert set(tr.phases.read()) == want, graph
        tr.close()


def test_wgrad_side_stream_matches_serial(monkeypatch):
    """Weight gradients on the side HIP stream (default) give bit-identical training to the
    fully serial schedule (DDLPC_WGRAD_STREAM=0): same kernels, only the overlap differs."""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    out = []
    for side in ("0", "1"):
        monkeypatch.setenv("DDLPC_WGRAD_STREAM", side)
        cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=4,
                          num_samples=1, test_holdout=0, impl="hip", accum_steps=2,
                          micro_streams=1)
        tr = Trainer(cfg, device=DEV)
        assert (tr.model._engine.side is not None) == (side == "1")
        batches = [device_random_batch(4, 64, 6, tr.device, seed=s) for s in range(4)]
        for i in range(3):
            tr.train_step([batches[i % 4], batches[(i + 1) % 4]])
        _sync()
        out.append(tr.flat.param_buf.clone())
        tr.close()
    assert torch.equal(out[0], out[1]), float((out[0] - out[1]).abs().max())


def test_hip_checkpoint_resume_is_exact(tmp_path):
    """Checkpoint save -> resume on the HIP path gives a bit-identical next step (weights are
    re-packed from the loaded fp32 masters; optimizer state and step counters restored)."""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer

    def cfg(**kw):
        return TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=4,
                           num_samples=1, test_holdout=0, impl="hip", **kw)
    tr = Trainer(cfg(), device=DEV)
    batches = [device_random_batch(4, 64, 6, tr.device, seed=s) for s in range(3)]
    tr.train_step([batches[0]])
    tr.train_step([batches[1]])
    path = tr.save(str(tmp_path / "ck.pt"))
    tr.train_step([batches[2]])
    _sync()
    want = tr.flat.param_buf.clone()
    want_state = {k: v.clone() for k, v in tr.model.state_dict().items()}
    tr.close()
    tr2 = Trainer(cfg(resume=path), device=DEV)
    assert tr2.step_count == 2 and tr2.optimizer.step_count == 2
    tr2.train_step([batches[2]])
    _sync()
    assert torch.equal(tr2.flat.param_buf, want), float((tr2.flat.param_buf - want).abs().max())
    for k, v in tr2.model.state_dict().items():      # BN running statistics too
        assert torch.equal(v, want_state[k]), k
    tr2.close()


def test_choose_schedule_times_both_and_keeps_faster():
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=4,
                      num_samples=1, test_holdout=0, impl="hip")
    tr = Trainer(cfg, device=DEV)
    r = tr.choose_schedule([device_random_batch(4, 64, 6, tr.device)], steps=2)
    assert set(r) == {"side_stream", "side_ms", "serial_ms", "side_rounds_ms",
                      "serial_rounds_ms", "side_alloc_retries", "serial_alloc_retries"}
    assert r["side_ms"] > 0 and r["side_alloc_retries"] == r["serial_alloc_retries"] == 0
    assert len(r["side_rounds_ms"]) == len(r["serial_rounds_ms"]) == 2
    eng = tr.model._engine
    assert (eng.side is not None) == r["side_stream"]
    # (no allocator retries at this size: the faster best round decides)
    assert (r["side_ms"] <= r["serial_ms"]) == r["side_stream"]
    assert tr.optimizer.step_count == 12
    tr.close()


def test_hip_grad_accumulation_matches_fp32_oracle():
    """accum_steps > 1 on the HIP path: the kernels ADD the second micro-batch's weight
    gradients into the flat buffer (direct grads, incl. the padded first-layer path).
    (a) the accumulated buffer equals the sum of the two micro-batches' separate HIP
    gradients; (b) it is as close to the fp32 oracle's accumulated gradient as stock
    PyTorch bf16 autocast is."""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.models import UNet
    from ddlpc.train.trainer import Trainer
    cfg = TrainConfig(model=ModelConfig(out_classes=6, depth=4), tile=64, batch_per_gpu=4,
                      num_samples=1, test_holdout=0, impl="hip", accum_steps=2)
    tr = Trainer(cfg, device=DEV)
    ref = UNet(out_classes=6, depth=4).to(DEV)
    ref.load_state_dict(tr.model.state_dict())
    amp = copy.deepcopy(ref)
    mb = [device_random_batch(4, 64, 6, tr.device, seed=s) for s in (1, 2)]
    sep = []
    for x, y in mb:                                    # each micro-batch alone
        tr.optimizer.zero_grad()
        loss, _ = tr.model.loss_and_correct(x, y)
        loss.backward()
        _sync()
        sep.append(tr.flat.grad_buf.clone())
    tr.optimizer.zero_grad()
    for x, y in mb:                                    # accumulated
        loss, _ = tr.model.loss_and_correct(x, y)
        loss.backward()
    _sync()
    acc = tr.flat.grad_buf.clone()
    assert float((acc - (sep[0] + sep[1])).abs().max()) <= 1e-6 * float(acc.abs().max())
    for x, y in mb:
        F.cross_entropy(ref(x.float().contiguous()), y).backward()
        with torch.autocast(DEV, dtype=torch.bfloat16):
            F.cross_entropy(amp(x.float().contiguous()).float(), y).backward()
    bad = []
    for (n, pr), (_, pa), (_, ph) in zip(ref.named_parameters(), amp.named_parameters(),
                                          tr.model.named_parameters()):
        if n.endswith((".0.bias", ".3.bias")) and "double_conv.double_conv" in n:
            continue
        ch, ca = _cos(pr.grad, ph.grad), _cos(pr.grad, pa.grad)
        if ch < min(0.98, ca - 0.08):
            bad.append((n, ch, ca))
    tr.close()
    assert not bad, bad


def test_recompute_matches_stored_activations():
    """cfg.recompute: block conv outputs are recomputed in backward instead of
    kept (1: first conv, 2: both where the block output is materialised).  Same kernels, same
    inputs -> the same bits: two optimizer steps at every level from the same init end in
    identical parameters, each level with less peak memory than the one below."""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    out = {}
    for rc in (0, 1, 2):
        cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=128, batch_per_gpu=8,
                          num_samples=1, test_holdout=0, impl="hip", recompute=rc)
        tr = Trainer(cfg, device=DEV)
        batches = [device_random_batch(8, 128, 6, tr.device, seed=40 + j) for j in range(2)]
        import gc
        gc.collect()                     # the previous trainer's tensors are gone before base
        _sync()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for b in batches:
            tr.train_step([b])
        _sync()
        # peak above what was resident before the steps (the other trainer's state and the
        # batches count in both runs alike)
        out[rc] = (tr.flat.param_buf.clone(), torch.cuda.max_memory_allocated() - base)
        tr.close()
        del tr, batches
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][0], out[2][0])
    # level 2 drops y2 only where the block output is materialised; with deferred skips
    # (default) the encoder y2 IS the skip and stays, so level 2 may equal level 1
    assert out[1][1] < out[0][1] and out[2][1] <= out[1][1] + (2 << 20), (out[0][1], out[1][1], out[2][1])


def test_deferred_skips_match_materialised_engine():
    """Engine level: with the encoder skips handed out pre-BN (engine.defer_skip = True, opt-in)
    a training step gives bit-identical loss and gradients to materialised skips."""
    from ddlpc.models.unet import UNet
    torch.manual_seed(3)
    model = UNet(out_classes=6).to(DEV)
    x = torch.rand(2, 3, 64, 64, device=DEV)
    y = torch.randint(0, 6, (2, 64, 64), device=DEV)
    res = {}
    for flag in (False, True):
        m = copy.deepcopy(model).to_hip()
        m._engine.defer_skip = flag
        assert any(m._engine.defer_skip_levels(x)) == flag
        loss, _ = m.loss_and_correct(x, y)
        loss.backward()
        res[flag] = (loss.detach(), [p.grad.clone() for p in m.parameters()])
    assert torch.equal(res[False][0], res[True][0])
    for g0, g1 in zip(res[False][1], res[True][1]):
        assert torch.equal(g0, g1)


def test_bf16_hip_training_curve_tracks_fp32_reference():
    """The reference trains in fp32 with no autocast (ref.py:702-704,754-756); the HIP engine
    computes in bf16 with fp32 master weights and fp32 Adam.  Same synthetic stream (same
    samples in the same order), 200 optimizer steps: HIP bf16 vs stock-PyTorch fp32
    (``impl="torch", dtype="fp32"``) from the SAME init, and a second fp32 run from ANOTHER
    init as the yardstick.  The bf16-vs-fp32 gap of the final train loss (mean of the last 20
    steps), held-out pixel accuracy and mIoU must stay within twice the fp32 seed-to-seed
    spread (floors 0.02 / 0.01 / 0.02 for a run where the two seeds happen to agree)."""
    import os
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")   # fp32 MIOpen: heuristic kernel choice
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.train.trainer import Trainer
    steps, B = 200, 8
    res = {}
    data = None
    for name, impl, dtype, seed in (("hip", "hip", "bf16", 7), ("fp32", "torch", "fp32", 7),
                                    ("fp32_seed8", "torch", "fp32", 8)):
        cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=B,
                          num_samples=steps * B, test_holdout=64, impl=impl, dtype=dtype,
                          seed=seed)
        tr = Trainer(cfg, device=DEV)
        assert tr.impl == impl and tr.autocast is False
        if impl == "hip":
            tr.model._engine.set_side_stream(False)
        elif data is None:
            data = (tr.train_set, tr.test_set)           # the seed-7 stream (NCHW layout)
        else:
            tr.train_set, tr.test_set = data             # another init, the same samples
        losses = []
        for i in range(steps):
            idx = list(range(i * B, (i + 1) * B))
            tr.train_step([tr._to_device(*tr.train_set.get(idx))])
            if i >= steps - 20:
                losses.append(tr.meter.reduce()["loss"])
            tr.meter.reset()
        v = tr.validate(batch=16)
        res[name] = (sum(losses) / len(losses), v["val_pixel_acc"], v["val_miou"])
        tr.close()
    print("final (train loss, val acc, val mIoU):", res)
    (lh, ah, mh), (lf, af, mf), (l8, a8, m8) = res["hip"], res["fp32"], res["fp32_seed8"]
    assert lf < 1.0 and l8 < 1.0, res                # the fp32 references actually learned
    assert abs(lh - lf) <= max(2 * abs(l8 - lf), 0.02), res
    assert abs(ah - af) <= max(2 * abs(a8 - af), 0.01), res
    assert abs(mh - mf) <= max(2 * abs(m8 - mf), 0.02), res


def test_concurrent_micro_streams_match_sequential_accumulation():
    """micro_streams > 1 (accumulation micro-batches on several HIP streams at once, the
    batch-1 reference regime): the per-micro-batch losses and the BatchNorm running
    statistics are bit-identical to the one-by-one loop (deferred running-stat updates
    applied in order) and the accumulated gradient equals the sequential one up to fp32
    summation order."""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    res = {}
    for ms in (1, 3):
        cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=2,
                          num_samples=1, test_holdout=0, impl="hip", micro_streams=ms,
                          accum_steps=7, bn_window=0)
        tr = Trainer(cfg, device=DEV)
        mbs = [device_random_batch(2, 64, 6, tr.device, seed=100 + j) for j in range(6)]
        tr.optimizer.zero_grad()
        if ms > 1:
            tr._concurrent_micros(mbs)
        else:
            for x, y in mbs:
                tr._micro(x, y, sync=False)
        _sync()
        res[ms] = (tr.flat.grad_buf.clone(), tr.meter.buf.clone(),
                   {k: v.clone() for k, v in tr.model.state_dict().items()
                    if "running" in k or "num_batches" in k})
        tr.train_step(mbs + [mbs[0]])              # and a full step through train_step
        _sync()
        assert torch.isfinite(tr.flat.param_buf).all()
        assert tr.micro_count == 13
        tr.close()
    (g1, m1, b1), (g3, m3, b3) = res[1], res[3]
    scale = float(g1.abs().max())
    assert torch.equal(m1, m3), (m1, m3)                 # identical per-micro-batch losses
    for k in b1:
        assert torch.equal(b1[k], b3[k]), k              # running stats / counters
    assert float((g1 - g3).abs().max()) <= 1e-5 * scale, float((g1 - g3).abs().max())


def test_concurrent_micro_stream_graphs():
    """hip_graph + micro_streams: every stream replays its own captured micro-batch graph
    (own static inputs, gradient buffer, BN slot, meter).  Training matches the one-by-one
    eager schedule to fp32 rounding over several optimizer steps."""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.train.trainer import Trainer
    out = {}
    for graph, ms in ((False, 1), (True, 3)):
        cfg = TrainConfig(model=ModelConfig(out_classes=6), tile=64, batch_per_gpu=1,
                          num_samples=1, test_holdout=0, impl="hip", micro_streams=ms,
                          accum_steps=8, hip_graph=graph, bn_window=0)
        tr = Trainer(cfg, device=DEV)
        batches = [device_random_batch(1, 64, 6, tr.device, seed=s) for s in range(9)]
        losses, grads = [], []
        step0 = tr.optimizer.step

        def step_capture(*a, _s=step0, _tr=tr, **k):
            grads.append(_tr.flat.grad_buf.clone())
            return _s(*a, **k)
        tr.optimizer.step = step_capture
        for i in range(5):
            tr.train_step([batches[(i + j) % 9] for j in range(8)])
            losses.append(tr.meter.reduce()["loss"])
            tr.meter.reset()
        _sync()
        if graph:
            assert all(g is not None for g in tr._ms_graphs), "micro-batch graphs not captured"
            assert "last" in tr._graphs
        assert tr.micro_count == 40 and tr.optimizer.step_count == 5
        out[graph] = (grads[0], losses)
        tr.close()
    (g0, l0), (g1, l1) = out[False], out[True]
    assert max(abs(a - b) for a, b in zip(l0, l1)) < 1e-3 * max(l0), (l0, l1)
    # the first step's exchanged gradient (same weights): equal up to fp32 summation order
    # (an Adam parameter bound would not do: every step moves a parameter by ~lr whatever
    # the gradient)
    scale = float(g0.abs().max())
    assert scale > 0 and float((g0 - g1).abs().max()) <= 1e-5 * scale, float((g0 - g1).abs().max())


@pytest.mark.parametrize("tile,accum,bpg,wd", [(512, 50, 1, 2), (64, 6, 2, 2), (128, 4, 1, 1)])
def test_bn_group_window_matches_sequential_micro_batches(tile, accum, bpg, wd):
    """The reference's regime (512^2, batch 1, 50 accumulated micro-batches, ref.py:685-687,
    750-766) as ONE batched pass with per-micro-batch BatchNorm groups, and the standard
    U-Net widths (width divisor 1, ref.py:687: 512 pooled channels at the deepest encoder
    levels) at 128^2.  Three independent yardsticks:

    * the same micro-batches one by one through the unfused grouped kernels
      (``bn_groups = 1``): where the batched convs tile like the batch-2 ones (64^2) the
      plain grouped window (no group fusions) must agree to fp32 summation order (rel L2
      <= 1e-5; measured 6.7e-8) with bit-identical running statistics, and the fused window
      (group-major conv statistics / prologues, the per-group deferred head) must stay
      within rel L2 5e-3 / cosine 0.999 of it; elsewhere FIXED bounds (rel L2 <= 3e-2,
      conv-weight cosine >= 0.9; measured at 512^2 x 50: 7.0e-3 / 0.909);
    * the fused one-by-one path (deferred BN, prologue fusion): rel L2 <= 8e-2, conv-weight
      cosine >= 0.85 (the same distance as fused vs unfused one by one, see below);
    * (small cases) the stock fp32 PyTorch model run micro-batch by micro-batch with its own
      train-mode BatchNorm: every gradient tensor as close to it as stock bf16 autocast is
      (cosine >= min(0.98, autocast - 0.08)) — no dependence on the new kernels."""
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.models import UNet
    from ddlpc.train.trainer import Trainer
    cfg = TrainConfig(model=ModelConfig(out_classes=6, width_divisor=wd), tile=tile,
                      batch_per_gpu=bpg, num_samples=1, test_holdout=0, impl="hip",
                      micro_streams=1, accum_steps=accum, bn_window=0)
    tr = Trainer(cfg, device=DEV)
    eng = tr.model._engine
    assert eng.bn_groups_supported(tile)
    mbs = [device_random_batch(bpg, tile, 6, tr.device, seed=300 + j) for j in range(accum)]
    bufs = {k: v for k, v in tr.model.state_dict().items() if "running" in k or "num_batches" in k}
    b0 = {k: v.clone() for k, v in bufs.items()}
    oracle = tile <= 128
    if oracle:
        ref = UNet(out_classes=6, width_divisor=wd).to(DEV)
        ref.load_state_dict(tr.model.state_dict())
        amp = copy.deepcopy(ref)

    def run(mode):
        tr.optimizer.zero_grad()
        tr.meter.reset()
        for k, v in bufs.items():
            v.copy_(b0[k])
        if mode in ("window", "window_plain", "window_lo"):
            # window_plain: the round-4 grouped path (no conv / head fusion of the groups);
            # window_lo: the group fusions engaged down to 2048 pixels per group (at 64^2 x 2
            # the default 16384 leaves every level unfused)
            keep = eng.group_fuse_min_px
            if mode == "window_plain":
                eng.group_fuse_min_px = None
            elif mode == "window_lo":
                eng.group_fuse_min_px = 2048
            try:
                tr._window_step(mbs, accum)              # one batched pass
            finally:
                eng.group_fuse_min_px = keep
        else:
            for x, y in mbs:                             # one by one
                eng.bn_groups = 1 if mode == "unfused" else 0
                try:
                    tr._micro(x, y, sync=False)
                finally:
                    eng.bn_groups = 0
        _sync()
        return (tr.flat.grad_buf.clone(), tr.meter.buf.clone(),
                {k: v.clone() for k, v in bufs.items()})

    modes = ("fused", "unfused", "window_plain", "window") + (("window_lo",) if tile == 64 else ())
    res = {m: run(m) for m in modes}
    assert eng.bn_groups == 0

    def compare(ref_mode, got):
        """-> (rel L2 over the whole gradient, min cosine over the conv weight tensors).
        (BatchNorm affine gradients — 1-D sums of many cancelling terms — are printed but
        not bounded per tensor: two equivalent one-by-one paths already differ there by a
        cosine of 0.89 at 512^2 x 50, measured)"""
        g0, g1 = res[ref_mode][0], res[got][0]
        rel = float((g1 - g0).norm() / g0.norm())
        cmin, worst, c1d = 1.0, None, 1.0
        for p in tr.flat.order:
            a, b = tr.flat.span(p)
            if float(g0[a:b].norm()) > 1e-3 * float(g0.norm()) / len(tr.flat.order):
                c = _cos(g1[a:b], g0[a:b])
                if p.dim() == 1:
                    c1d = min(c1d, c)
                elif c < cmin:
                    cmin, worst = c, tuple(p.shape)
        print(f"{got} vs {ref_mode}: rel L2 {rel:.3e}, min conv-weight cos {cmin:.6f} {worst}, "
              f"min 1-D cos {c1d:.4f}")
        return rel, cmin

    rel_u, cos_u = compare("unfused", "window")
    rel_f, cos_f = compare("fused", "window")
    rel_p, cos_p = compare("unfused", "window_plain")
    rel_w, cos_w = compare("window_plain", "window")     # the group fusions (conv tiles, head)
    compare("fused", "unfused")                          # (the two one-by-one paths, printed)
    # fixed bounds.  Measured (rel L2 / min conv-weight cosine): window vs unfused 4.6e-3 /
    # 0.959 at 512^2 x 50, 1.9e-2 / 0.944 at 128^2 width-divisor 1; window vs fused 7.0e-3 /
    # 0.910, 5.2e-2 / 0.912 (64^2), 2.7e-2 / 0.907 (128^2) — and the two one-by-one paths
    # differ from each other by exactly as much: the deepest weight gradients of a small-
    # batch U-Net, whose bottleneck BatchNorms normalise 2x2 .. 16x16 pixels, amplify bf16
    # rounding differences.  (The fp32 yardstick below is the kernel-independent check.)
    # (64^2: the plain grouped window runs the same arithmetic as the one-by-one unfused
    # path; the fused window moves the head's BN (deferred, per-group) and, from 16384 pixels
    # per group, the conv statistics to other rounding points: measured 1.5e-3 / 0.99994)
    if tile == 64:
        assert rel_p <= 1e-5, rel_p
        assert rel_w <= 5e-3 and cos_w >= 0.999, (rel_w, cos_w)
        # the group-major conv statistics, per-group prologues and grouped conv3_bwd32 engaged
        # (window_lo).  Their forward statistics come from the fp32 conv outputs, the plain
        # path's from the stored bf16 y, so the gradients differ as much as the two
        # equivalent one-by-one paths do (measured 5.2e-2 / 0.906, the bottleneck BatchNorms
        # of 2 x 2 x 2 pixels amplify it); the forward is held tightly: every group's
        # statistics (the running statistics after the G in-order updates) and the loss — a
        # mis-assigned group row would be off by the whole spread between micro-batches
        rel_l, cos_l = compare("window_plain", "window_lo")
        assert rel_l <= 8e-2 and cos_l >= 0.85, (rel_l, cos_l)
        ml, mp = res["window_lo"][1], res["window_plain"][1]
        assert abs(float(ml[0] - mp[0])) <= 1e-3 * float(mp[0]), (ml, mp)
        for k in b0:
            if "running_mean" in k:
                bl, bp = res["window_lo"][2][k], res["window_plain"][2][k]
                std = res["window_plain"][2][k.replace("running_mean", "running_var")].sqrt()
                assert torch.all((bl - bp).abs() <= 1e-2 * (bp.abs() + std)), k
            elif "running_var" in k:
                assert torch.allclose(res["window_lo"][2][k], res["window_plain"][2][k],
                                      rtol=1e-2, atol=0), k
    else:
        assert rel_u <= 3e-2 and cos_u >= 0.9, (rel_u, cos_u)
        assert rel_p <= 3e-2 and cos_p >= 0.9, (rel_p, cos_p)
    assert rel_f <= 8e-2 and cos_f >= 0.85, (rel_f, cos_f)
    for ref_mode in ("unfused", "fused"):
        m0, m1 = res[ref_mode][1], res["window"][1]
        assert m1[2] == m0[2] and m1[3] == m0[3] == accum, (m0, m1)
        assert abs(float(m1[0] - m0[0])) <= 2e-3 * float(m0[0]), (ref_mode, m0, m1)
        assert abs(float(m1[1] - m0[1])) <= 2e-3 * float(m0[2]), (ref_mode, m0, m1)
    for k in b0:
        bu, bw, bf = res["unfused"][2][k], res["window"][2][k], res["fused"][2][k]
        if "num_batches" in k or tile == 64:
            bp = res["window_plain"][2][k]
            assert torch.equal(bp, bu), (k, float((bp.float() - bu.float()).abs().max()))
        if "num_batches" in k:
            assert torch.equal(bw, bf), k
        else:
            # per-micro-batch means / variances of conv outputs that round to bf16
            # independently (the batched convs tile differently; on the fused levels the
            # window's statistics come from the fp32 conv outputs before the bf16 store, the
            # unfused path's from the stored bf16 y): measured up to 2.3e-4 on the
            # bottleneck's running means of magnitude ~1 (256 pixels per micro-batch), 2.1e-3
            # on a 64-pixel bottleneck running variance at 128^2 width divisor 1
            err = float((bw - bu).abs().max())
            assert err <= 5e-3 * max(1.0, float(bu.abs().max())), (k, err)
    if oracle:
        # fp32 stock model (and bf16 autocast), micro-batch by micro-batch, own BatchNorm each
        for x, y in mbs:
            F.cross_entropy(ref(x.float().contiguous()), y).backward()
            with torch.autocast(DEV, dtype=torch.bfloat16):
                F.cross_entropy(amp(x.float().contiguous()).float(), y).backward()
        gw = res["window"][0]
        bad, worst = [], []
        for (n, pr), (_, pa), ph in zip(ref.named_parameters(), amp.named_parameters(),
                                        tr.model.parameters()):
            if n.endswith((".0.bias", ".3.bias")) and "double_conv.double_conv" in n:
                continue
            a, b = tr.flat.span(ph)
            ch, ca = _cos(pr.grad, gw[a:b]), _cos(pr.grad, pa.grad)
            worst.append((ch - ca, n, ch, ca))
            if ch < min(0.98, ca - 0.08):
                bad.append((n, ch, ca))
        print("window vs fp32, worst cosine deltas to autocast:", sorted(worst)[:3])
        assert not bad, bad
    # and a full optimizer step through train_step picks the window (auto)
    tr.cfg.bn_window = -1
    assert tr._window_size(accum) == (accum if bpg * tile * tile <= tr.SMALL_MICRO_PIXELS else 0)
    tr.train_step(mbs)
    _sync()
    assert torch.isfinite(tr.flat.param_buf).all()
    tr.close()
