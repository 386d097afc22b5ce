"""``grad_codec="powersgd"`` through the reducer and the Trainer on two gloo ranks (on a GPU both share
the one device): every exchange against the fp64 contract run on the gathered local gradients with
its own carried residuals and warm starts, within the bound of ``powersgd_cases.py``."""
import pytest
import torch

from dist_utils import run


def _psgd_rank(rank, world, device, reduce, overlap):
    import os
    os.environ["LOCAL_RANK"] = "0"              # both ranks on the box's single GPU
    import torch.distributed as dist
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.parallel import codec as C
    from ddlpc.train.trainer import Trainer
    from powersgd_cases import contract
    from update_cases import ulp32
    cfg = TrainConfig(model=ModelConfig(out_classes=6, width_divisor=2 if device == "cuda" else 4), tile=64,
                      batch_per_gpu=2, num_samples=1, test_holdout=0, impl="hip", backend="gloo", bucket_mb=1.0,
                      overlap_comm=overlap, grad_codec="powersgd", powersgd_rank=4, reduce=reduce)
    tr = Trainer(cfg, device=device)
    red, n = tr.reducer, tr.flat.grad_buf.numel()
    weights = C.reference_weights(world) if reduce == "reference" else [red.weight] * world
    state = {dt: ([torch.zeros(n, dtype=dt) for _ in range(world)],
                  [C.powersgd_init_q(b.psgd.plan, cfg.seed, b.idx).to(dt) for b in red.buckets])
             for dt in (torch.float64, torch.float32)}
    items = [(b.psgd.plan, slice(b.start, b.end)) for b in red.buckets]
    lows = [(b.start + off, nn * mm) for b in red.buckets for off, nn, mm, _, _ in b.psgd.plan.low.tolist()]
    raws = [(b.start + off, ln) for b in red.buckets for off, ln, _ in b.psgd.plan.raw.tolist()]
    out = {"same": [], "raw": [], "worst": 0.0, "lost": 0.0}
    for step in range(2):                       # two exchanges, no optimizer step in between
        x, y = device_random_batch(2, 64, 6, tr.device, seed=10 + rank + 100 * step)
        grads = []
        e0 = torch.zeros(n) if red.residual is None else red.residual.cpu().clone()
        for armed in (False, True):             # the local gradient, then the same one exchanged
            red.prepare(sync=armed)
            loss, _ = tr.model.loss_and_correct(x, y)
            loss.backward()
            if armed:
                launched = red.stats["launched_in_backward"]
                red.finish()
            grads.append(tr.flat.grad_buf.cpu().clone())    # (synchronises; a copy on the CPU too)
            tr.optimizer.zero_grad()
        gl, gx = ([torch.empty_like(grads[0]) for _ in range(world)] for _ in range(2))
        sent = [torch.empty(n, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(gl, grads[0])
        dist.all_gather(gx, grads[1])
        # this rank's w (A - e) of the kernels' own residuals, in double: the ranks' sum is the decoded gradient
        dist.all_gather(sent, weights[rank] * ((e0 + grads[0]).double() - red.residual.cpu().double()))
        out["same"].append(all(torch.equal(gx[0].view(torch.int32), t.view(torch.int32)) for t in gx))
        rawsum = sum(torch.tensor(w) * g for w, g in zip(weights, gl))
        out["raw"].append(all(torch.equal(grads[1][a:a + k], rawsum[a:a + k]) for a, k in raws))
        w64, w32 = (contract(items, gl, *state[dt], weights, dt)[0] for dt in (torch.float64, torch.float32))
        kept = sum(sent)
        for a, k in lows:
            ref = w64[a:a + k]
            bound = 8 * float((w32[a:a + k].double() - ref).norm()) + ulp32(float(ref.abs().max()))
            out["worst"] = max(out["worst"], float((grads[1][a:a + k].double() - ref).norm()) / bound)
            out["lost"] = max(out["lost"], float((kept[a:a + k] - grads[1][a:a + k].double()).norm()) / bound)
    for i in range(3):
        tr.train_step([device_random_batch(2, 64, 6, tr.device, seed=1000 * i + rank)])
    p = tr.flat.param_buf.cpu()
    ps = [torch.empty_like(p) for _ in range(world)]
    dist.all_gather(ps, p)
    out.update(launched=launched, buckets=len(red.buckets), wire=red.stats["powersgd_wire_floats"],
               plan_wire=sum(b.psgd.plan.wire_p + b.psgd.plan.wire_q for b in red.buckets),
               dense=red.stats["powersgd_dense_floats"], replicas_equal=all(torch.equal(ps[0], q) for q in ps))
    tr.close()
    return out


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("reduce", ["mean", "reference"])
@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_powersgd_two_ranks_contract_and_replicas(device, reduce, overlap):
    res = run(_psgd_rank, 2, (device, reduce, overlap), timeout=200)
    for r in (0, 1):
        o = res[r]
        print(f"powersgd dp {device} {reduce}: error / bound {o['worst']:.3f}, sum w (A - e) vs decoded {o['lost']:.3f}")
        assert o["buckets"] > 1 and o["launched"] == (2 * o["buckets"] if overlap else 0), o
        assert o["wire"] == o["plan_wire"] > 0 and o["wire"] < o["dense"], o
        assert o["same"] == [True, True] and o["raw"] == [True, True], o
        assert o["worst"] <= 1.0 and o["lost"] <= 1.0, o
        assert o["replicas_equal"], o
