"""Zoomed and rotated random crops on the CPU kernels (``csrc/cpu_ref.cpp``): ``warp_gather``
and ``warp_params`` against ``crop_gather``, their numpy twins and a closed form, the scene
data set, the configuration, and training from a directory of scenes (the bodies shared with
the GPU run live in ``warp_cases.py``)."""
import pytest

import warp_cases as wc

DEV = "cpu"


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


def test_config_and_cli_flags(tmp_path):
    wc.check_config_and_cli(tmp_path)


def test_fit_warped_scene_dir_and_resume(tmp_path):
    from ddlpc.config import ModelConfig
    # the smallest U-Net the engine accepts (widths 16, 32)
    wc.check_training(DEV, tmp_path, ModelConfig(out_classes=6, depth=2, width_divisor=4))


def test_cli_trains_with_zoom_and_rotation(tmp_path):
    from ddlpc.cli import main
    d = str(tmp_path / "scenes")
    wc.write_training_scenes(d)
    assert main(["train", "--data", "scene_dir", "--data-dir", d, "--augment", "d4", "--zoom-min", "0.5",
                 "--zoom-max", "2", "--rotate-deg", "30", "--tile", "32", "--depth", "2", "--width-divisor", "4",
                 "--test-holdout", "1", "--batch-per-gpu", "2", "--crops-per-epoch", "4", "--device", "cpu",
                 "--impl", "hip", "--log-every", "0"]) == 0
