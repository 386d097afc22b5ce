"""``python -m ddlpc predict --tta``: the flag reaches the predictor and ``predict.jsonl`` (CPU
kernels, a tiny checkpoint)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--tile", "32", "--depth", "3", "--device", "cpu", "--impl", "hip"]


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from ddlpc.cli import main
    ck = str(tmp_path_factory.mktemp("ck"))
    assert main(["train", *FLAGS, "--batch-per-gpu", "2", "--num-samples", "8", "--test-holdout", "2",
                 "--max-steps", "3", "--ckpt-dir", ck]) == 0
    return os.path.join(ck, sorted(os.listdir(ck))[-1])


def _predict(ckpt, scene, out_dir, *extra):
    r = subprocess.run([sys.executable, "-m", "ddlpc", "predict", *FLAGS, "--checkpoint", ckpt,
                        "--input", scene, "--out-dir", out_dir, *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    from PIL import Image
    records = [json.loads(s) for s in open(os.path.join(out_dir, "predict.jsonl"))]
    assert len(records) == 1
    return records[0], np.asarray(Image.open(os.path.join(out_dir, "s.png")))


def test_cli_predict_tta(checkpoint, tmp_path):
    from PIL import Image
    scene = str(tmp_path / "s.png")
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (45, 70, 3), dtype=np.uint8)).save(scene)
    rec_d4, pred_d4 = _predict(checkpoint, scene, str(tmp_path / "d4"), "--tta", "d4")
    rec_none, pred_none = _predict(checkpoint, scene, str(tmp_path / "none"), "--tta", "none")
    rec_def, pred_def = _predict(checkpoint, scene, str(tmp_path / "default"))
    assert rec_d4["tta"] == "d4" and rec_none["tta"] == "none" and rec_def["tta"] == "none"
    assert rec_d4["windows"] == rec_none["windows"] == 2 * 3
    assert pred_d4.shape == pred_none.shape == (45, 70)
    assert np.array_equal(pred_none, pred_def)
    assert not np.array_equal(pred_d4, pred_none)
