"""Augmented random crops on the CPU kernels (``csrc/cpu_ref.cpp``): ``crop_gather`` and
``crop_params`` against their numpy twins, the scene data set, training from a directory of
unequal scenes, and the configuration (the bodies shared with the GPU run live in
``crop_cases.py``)."""
import pytest

import crop_cases as cc

DEV = "cpu"


@pytest.mark.parametrize("tile,in_ch,cpad", cc.GATHER_CASES)
def test_crop_gather_matches_numpy_oracle(tile, in_ch, cpad):
    cc.check_gather(DEV, tile, in_ch, cpad)


def test_crop_gather_far_origins():
    cc.check_far_origins(DEV)


def test_crop_gather_rejects_bad_arguments():
    cc.check_gather_rejects(DEV)


def test_crop_gather_color():
    cc.check_color(DEV)


def test_crop_gather_identity_equals_tile_gather():
    cc.check_identity_equals_tile_gather(DEV)


def test_crop_params_matches_twin():
    cc.check_params(DEV)


def test_crop_params_distribution():
    cc.check_distribution(DEV)


def test_scene_dataset(tmp_path):
    cc.check_dataset(DEV, tmp_path)


def test_tiles_as_scenes_serve_d4_images_of_their_tiles(tmp_path):
    cc.check_tiles_as_scenes(DEV, tmp_path)


def test_fit_scene_dir_and_resume(tmp_path):
    from ddlpc.config import ModelConfig
    # the smallest U-Net the engine accepts (widths 16, 32)
    cc.check_training(DEV, tmp_path, ModelConfig(out_classes=6, depth=2, width_divisor=4))


def test_config_and_cli_flags(tmp_path):
    cc.check_config_and_cli(tmp_path)


def test_cli_trains_from_scene_dir(tmp_path):
    from ddlpc.cli import main
    d = str(tmp_path / "scenes")
    cc.write_training_scenes(d)
    assert main(["train", "--data", "scene_dir", "--data-dir", d, "--augment", "d4", "--tile", "32",
                 "--depth", "2", "--width-divisor", "4", "--test-holdout", "1", "--batch-per-gpu", "2",
                 "--crops-per-epoch", "4", "--device", "cpu", "--impl", "hip", "--log-every", "0"]) == 0


def test_vaihingen_dir_wraps_only_when_augmented(tmp_path):
    """``vaihingen_dir`` keeps the plain tile path unless an augmentation is asked for."""
    import numpy as np
    from ddlpc.data import SceneCropDataset, TileDataset
    from ddlpc.config import ModelConfig
    from ddlpc.train.trainer import Trainer
    d = str(tmp_path / "tiles")
    cc.write_scenes(d, {f"t{i}": (32, 32) for i in range(6)})
    kw = dict(data="vaihingen_dir", tile=32, test_holdout=2, crops_per_epoch=0, augment="none", gain_jitter=0.0,
              bias_jitter=0.0, model=ModelConfig(out_classes=6, depth=2, width_divisor=4), log_dir=None)
    tr = Trainer(cc.train_cfg(tmp_path, d, **kw), device=DEV)
    assert isinstance(tr.train_set, TileDataset) and isinstance(tr.test_set, TileDataset)
    tr.close()
    tr = Trainer(cc.train_cfg(tmp_path, d, **dict(kw, augment="flip")), device=DEV)
    assert isinstance(tr.train_set, SceneCropDataset) and len(tr.train_set) == 4
    assert isinstance(tr.test_set, SceneCropDataset) and len(tr.test_set) == 2
    p, _ = tr.train_set.crop_rows([0, 1, 2, 3])
    assert not p[:, 1:3].any() and int(p[:, 3].max()) <= 3
    held = TileDataset.from_dir(d, 2)[1]
    xa, ya = tr.test_set.get([0, 1])
    xb, yb = held.get([0, 1])
    assert np.array_equal(ya.numpy(), yb.numpy()) and (xa.float() == xb.bfloat16().float()).all()
    tr.close()
