"""Whole-scene prediction on the CPU kernels (``csrc/cpu_ref.cpp``): the window plan, the
three operators, ``ScenePredictor`` and ``python -m ddlpc predict`` end to end (the bodies
shared with the GPU run live in ``predict_cases.py``)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import predict_cases as pc
from dist_utils import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cpu"


@pytest.fixture(scope="module")
def models():
    return {name: pc.make_model(name, DEV) for name in pc.MODELS}


# ------------------------------------------------------------------ plan (no kernels)
@pytest.mark.parametrize("H,W,tile,overlap", pc.PLAN_CASES)
def test_plan_windows(H, W, tile, overlap):
    pc.check_plan(H, W, tile, overlap)


def test_cosine_weights_formula_and_minimum():
    from ddlpc.infer import blend_weights
    w = blend_weights(32, 16, "cosine").double()
    t = torch.arange(16, dtype=torch.float64)
    r = (0.5 - 0.5 * torch.cos(torch.pi * (t + 0.5) / 16)).float().double()
    assert torch.allclose(w[:16], r, atol=1e-7, rtol=0) and torch.equal(w[16:], w[:16].flip(0))
    assert torch.allclose(w[16:] + w[:16], torch.ones(16, dtype=torch.float64), atol=1e-7)
    core = blend_weights(32, 16, "core")
    assert torch.equal(core, torch.tensor([0.] * 8 + [1.] * 16 + [0.] * 8))
    assert abs(float(pc.weight_sum_map(70, 52, 32, 16, "cosine").min()) - 0.30) < 0.01


def test_reflect_rule():
    from ddlpc.infer import reflect
    assert [reflect(i, 4) for i in range(-7, 9)] == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert [reflect(i, 1) for i in (-3, 0, 5)] == [0, 0, 0]
    assert [reflect(i, 2) for i in range(-2, 4)] == [0, 1, 0, 1, 0, 1]


# ------------------------------------------------------------------ operators
@pytest.mark.parametrize("H,W,tile,overlap", pc.PLAN_CASES)
def test_window_gather(H, W, tile, overlap):
    pc.check_window_gather(DEV, H, W, tile, overlap)


@pytest.mark.parametrize("C,K", pc.HEAD_CASES)
def test_head_predict_accum(C, K):
    pc.check_head_predict_accum(DEV, C, K, "cosine")


def test_head_predict_accum_core_weights():
    pc.check_head_predict_accum(DEV, 32, 6, "core")


def test_head_predict_accum_rejects_bad_arguments():
    pc.check_head_predict_accum_rejects(DEV)


@pytest.mark.parametrize("K", [3, 6, 16])
def test_scene_finalize(K):
    pc.check_scene_finalize(DEV, K)


# ------------------------------------------------------------------ predictor
@pytest.mark.parametrize("blend", ["cosine", "core"])
@pytest.mark.parametrize("H,W,tile,overlap", pc.PREDICTOR_SHAPES)
@pytest.mark.parametrize("name", list(pc.MODELS))
def test_predictor_fused_matches_unfused(models, name, H, W, tile, overlap, blend):
    pc.check_predictor_fused_vs_unfused(DEV, models[name], H, W, tile, overlap, blend)


@pytest.mark.parametrize("H,W,tile,overlap", pc.PREDICTOR_SHAPES)
@pytest.mark.parametrize("name", list(pc.MODELS))
def test_predictor_against_fp32_modules(models, name, H, W, tile, overlap):
    pc.check_predictor_vs_fp32(DEV, models[name], H, W, tile, overlap)


@pytest.mark.parametrize("name", list(pc.MODELS))
def test_single_window_matches_model_forward(models, name):
    pc.check_single_window_matches_forward(DEV, models[name])


def test_predictor_rejects_bad_arguments(models):
    pc.check_predictor_arguments(DEV, models["d3_convt"])


# ------------------------------------------------------------------ end to end
FLAGS = ["--tile", "32", "--depth", "3", "--device", "cpu", "--impl", "hip"]
SCENES = {"s0": (45, 70), "s1": (61, 38)}                 # no multiples of the tile or stride


def _write_scenes(path, labels):
    from PIL import Image
    os.makedirs(path)
    g = np.random.default_rng(0)
    for stem, (h, w) in SCENES.items():
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(path, stem + ".png"))
        if labels:
            np.save(os.path.join(path, stem + "_label.npy"), g.integers(0, 6, (h, w), dtype=np.uint8))


def _cli_predict(ckpt, inputs, out_dir, env=None):
    r = subprocess.run([sys.executable, "-m", "ddlpc", "predict", *FLAGS, "--checkpoint", ckpt,
                        "--input", inputs, "--out-dir", out_dir, "--window-batch", "3", "--save-proba"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _rank_predict(rank, world, ckpt, inputs, out_dir):
    from ddlpc.config import ModelConfig, TrainConfig
    from ddlpc.infer import predict
    cfg = TrainConfig(model=ModelConfig(depth=3), tile=32, impl="hip", timeout_s=60)
    return predict(cfg, ckpt, inputs, out_dir, device="cpu", window_batch=3)


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from ddlpc.cli import main
    ck = str(tmp_path_factory.mktemp("ck"))
    assert main(["train", *FLAGS, "--batch-per-gpu", "2", "--num-samples", "8", "--test-holdout", "2",
                 "--max-steps", "3", "--ckpt-dir", ck]) == 0
    return os.path.join(ck, sorted(os.listdir(ck))[-1])


def test_cli_predict_end_to_end(checkpoint, tmp_path):
    from PIL import Image
    inputs, out = str(tmp_path / "scenes"), str(tmp_path / "out")
    _write_scenes(inputs, labels=True)
    summary = _cli_predict(checkpoint, inputs, out)
    assert summary["cmd"] == "predict" and summary["scenes"] == 2
    assert summary["pixels"] == sum(h * w for h, w in SCENES.values())
    hits = 0
    for stem, (h, w) in SCENES.items():
        pred = np.asarray(Image.open(os.path.join(out, stem + ".png")))
        assert pred.shape == (h, w) and pred.dtype == np.uint8 and int(pred.max()) < 6
        assert np.asarray(Image.open(os.path.join(out, stem + "_color.png"))).shape == (h, w, 3)
        proba = np.load(os.path.join(out, stem + "_proba.npy"))
        assert proba.shape == (6, h, w) and proba.dtype == np.float16
        assert float((proba.argmax(0) == pred).mean()) > 0.99      # (fp16 rounding ties)
        hits += int((pred == np.load(os.path.join(inputs, stem + "_label.npy"))).sum())
    assert abs(summary["pixel_acc"] - hits / summary["pixels"]) < 1e-12
    assert len(summary["iou"]) == 6 and 0.0 <= summary["miou"] <= 1.0
    lines = [json.loads(s) for s in open(os.path.join(out, "predict.jsonl"))]
    assert [r["name"] for r in lines] == ["s0.png", "s1.png"]
    for r, (h, w) in zip(lines, SCENES.values()):
        assert {"name", "H", "W", "windows", "ms", "pixel_acc", "iou"} <= set(r)
        assert (r["H"], r["W"]) == (h, w) and r["windows"] == -(-h // 24) * -(-w // 24)

    # a 2-rank gloo world writes the same bytes and reports the same summary
    out2 = str(tmp_path / "out2")
    res = run(_rank_predict, world=2, args=(checkpoint, inputs, out2), timeout=240)
    for k, v in res[0].items():
        assert summary[k] == v, k
    assert res[1] == res[0]
    for stem in SCENES:
        for suffix in (".png", "_color.png"):
            with open(os.path.join(out, stem + suffix), "rb") as f0, \
                    open(os.path.join(out2, stem + suffix), "rb") as f1:
                assert f0.read() == f1.read()
    assert len(open(os.path.join(out2, "predict.jsonl")).readlines()) == 2


def test_cli_predict_without_labels(checkpoint, tmp_path):
    inputs, out = str(tmp_path / "scenes"), str(tmp_path / "out")
    _write_scenes(inputs, labels=False)
    summary = _cli_predict(checkpoint, inputs, out)
    assert summary["scenes"] == 2 and "pixel_acc" not in summary and "miou" not in summary
    lines = [json.loads(s) for s in open(os.path.join(out, "predict.jsonl"))]
    assert len(lines) == 2 and all("pixel_acc" not in r for r in lines)
    single = _cli_predict(checkpoint, os.path.join(inputs, "s1.png"), str(tmp_path / "one"))
    assert single["scenes"] == 1 and single["pixels"] == 61 * 38
