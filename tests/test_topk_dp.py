"""``grad_codec="topk"`` through the bucketed reducer and the Trainer on two gloo ranks (on a GPU
both ranks share the one device): every exchange must leave exactly the CPU oracle's gradient on
every rank — per-rank residuals carried from one exchange to the next — and replicas identical."""
import pytest
import torch

from dist_utils import run


def _topk_rank(rank, world, device, reduce, overlap):
    import os
    os.environ["LOCAL_RANK"] = "0"              # both ranks on the box's single GPU
    import torch.distributed as dist
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.data import device_random_batch
    from ddlpc.parallel import codec as C
    from ddlpc.train.trainer import Trainer
    # the CPU kernels get the narrowest U-Net the engine takes (8.7 MB of gradients)
    cfg = TrainConfig(model=ModelConfig(out_classes=6, width_divisor=2 if device == "cuda" else 4), tile=64, batch_per_gpu=2, num_samples=1,
                      test_holdout=0, impl="hip", backend="gloo", bucket_mb=1.0, overlap_comm=overlap,
                      grad_codec="topk", topk_ratio=0.05, reduce=reduce)
    tr = Trainer(cfg, device=device)
    red = tr.reducer
    sync = torch.cuda.synchronize if device == "cuda" else (lambda: None)
    weights = C.reference_weights(world) if reduce == "reference" else [red.weight] * world
    residual = [torch.zeros(tr.flat.grad_buf.numel()) for _ in range(world)]      # the oracle's
    exact, ks = [], [C.topk_count(b.end - b.start, 0.05) for b in red.buckets]
    for step in range(2):                       # two exchanges, no optimizer step in between
        x, y = device_random_batch(2, 64, 6, tr.device, seed=10 + rank + 100 * step)
        grads = []
        for armed in (False, True):             # the local gradient, then the same one exchanged
            red.prepare(sync=armed)
            loss, _ = tr.model.loss_and_correct(x, y)
            loss.backward()
            if armed:
                launched = red.stats["launched_in_backward"]
                red.finish()
            sync()
            grads.append(tr.flat.grad_buf.cpu())
            tr.optimizer.zero_grad()
        gl = [torch.empty_like(grads[0]) for _ in range(world)]
        dist.all_gather(gl, grads[0])
        want = torch.zeros_like(grads[0])
        for b, k in zip(red.buckets, ks):
            enc = [C.topk_encode(g[b.start:b.end], e[b.start:b.end], k) for g, e in zip(gl, residual)]
            C.topk_decode_sum(want[b.start:b.end], [i for i, _ in enc], [v for _, v in enc], weights)
        exact.append(torch.equal(grads[1].view(torch.int32), want.view(torch.int32)))
    for i in range(3):
        tr.train_step([device_random_batch(2, 64, 6, tr.device, seed=1000 * i + rank)])
    sync()
    p = tr.flat.param_buf.cpu()
    ps = [torch.empty_like(p) for _ in range(world)]
    dist.all_gather(ps, p)
    out = {"exact": exact, "launched": launched, "buckets": len(red.buckets),
           "topk_k": red.stats["topk_k"], "sum_k": sum(ks),
           "replicas_equal": all(torch.equal(ps[0], q) for q in ps)}
    tr.close()
    return out


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("reduce", ["mean", "reference"])
@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_topk_two_ranks_oracle_and_replicas(device, reduce, overlap):
    res = run(_topk_rank, 2, (device, reduce, overlap), timeout=200)
    for r in (0, 1):
        o = res[r]
        assert o["buckets"] > 1 and o["launched"] == (2 * o["buckets"] if overlap else 0), o
        assert o["topk_k"] == o["sum_k"] > 0, o
        assert o["exact"] == [True, True], o
        assert o["replicas_equal"], o
