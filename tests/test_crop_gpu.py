"""Augmented random crops on the gfx950 kernels (``csrc/data.hip``): the bodies live in
``crop_cases.py`` and also run on the CPU kernels (``test_crop_cpu.py``)."""
import pytest

import crop_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def test_scene_dataset(tmp_path):
    cc.check_dataset(DEV, tmp_path)


def test_tiles_as_scenes_serve_d4_images_of_their_tiles(tmp_path):
    cc.check_tiles_as_scenes(DEV, tmp_path)


def test_fit_scene_dir_and_resume(tmp_path):
    from ddlpc.config import ModelConfig
    cc.check_training(DEV, tmp_path, ModelConfig(out_classes=6))
