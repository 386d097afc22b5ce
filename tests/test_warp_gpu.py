"""Zoomed and rotated random crops on the gfx950 kernels (``csrc/data.hip``): the bodies live
in ``warp_cases.py`` and also run on the CPU kernels (``test_warp_cpu.py``)."""
import pytest

import warp_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("tile,in_ch,cpad", wc.GATHER_CASES)
def test_warp_gather_identity_equals_crop_gather(tile, in_ch, cpad):
    wc.check_identity(DEV, tile, in_ch, cpad)


@pytest.mark.parametrize("tile,in_ch,cpad", wc.GATHER_CASES)
def test_warp_gather_quarter_turns_equal_crop_codes(tile, in_ch, cpad):
    wc.check_quarter_turns(DEV, tile, in_ch, cpad)


@pytest.mark.parametrize("tile,in_ch,cpad", wc.GATHER_CASES)
def test_warp_gather_matches_numpy_oracle(tile, in_ch, cpad):
    wc.check_twin(DEV, tile, in_ch, cpad)


def test_warp_gather_keeps_a_constant_image():
    wc.check_constant_image(DEV)


def test_warp_gather_ramp_is_the_coordinate():
    wc.check_ramp(DEV)


def test_warp_params_matches_twin_and_crop_params():
    wc.check_params(DEV)


def test_warp_ops_reject_bad_arguments():
    wc.check_rejects(DEV)


def test_warped_scene_dataset(tmp_path):
    wc.check_dataset(DEV, tmp_path)


def test_fit_warped_scene_dir_and_resume(tmp_path):
    from ddlpc.config import ModelConfig
    wc.check_training(DEV, tmp_path, ModelConfig(out_classes=6))
