"""Test-time augmentation of whole-scene prediction on the CPU kernels (``csrc/cpu_ref.cpp``):
``window_gather`` / ``head_predict_accum`` with symmetry codes and ``ScenePredictor(tta=...)``
(the bodies shared with the GPU run live in ``tta_cases.py``)."""
import pytest

import predict_cases as pc
import tta_cases as tc

DEV = "cpu"


@pytest.fixture(scope="module")
def models():
    return {name: pc.make_model(name, DEV) for name in pc.MODELS}


@pytest.mark.parametrize("H,W,tile", tc.GATHER_CASES)
def test_window_gather_codes(H, W, tile):
    tc.check_window_gather_codes(DEV, H, W, tile)


@pytest.mark.parametrize("in_ch,cpad", tc.CHANNEL_CASES)
def test_window_gather_channels(in_ch, cpad):
    tc.check_window_gather_channels(DEV, in_ch, cpad)


@pytest.mark.parametrize("blend", ["cosine", "core"])
@pytest.mark.parametrize("C,K", pc.HEAD_CASES)
def test_head_predict_accum_codes(C, K, blend):
    tc.check_head_predict_accum_codes(DEV, C, K, blend)


def test_round_trip_without_network():
    tc.check_round_trip(DEV)


@pytest.mark.parametrize("tta", ["flip", "d4"])
@pytest.mark.parametrize("H,W,tile,overlap", tc.TTA_SHAPES)
@pytest.mark.parametrize("name", list(pc.MODELS))
def test_predictor_tta_fused_matches_unfused(models, name, H, W, tile, overlap, tta):
    tc.check_predictor_tta(DEV, models[name], H, W, tile, overlap, tta)


def test_predictor_tta_window_batch_below_views(models):
    tc.check_predictor_tta(DEV, models["d2_bilinear"], 33, 95, 32, 0, "d4", window_batch=3)


@pytest.mark.parametrize("tta,group", [("d4", (1, 2, 4, 7)), ("flip", (1, 2, 3))])
@pytest.mark.parametrize("H,tile,overlap", [(H, t, o) for H, _, t, o in tc.EQUIVARIANCE_SHAPES])
@pytest.mark.parametrize("name", list(pc.MODELS))
def test_tta_prediction_is_equivariant(models, name, H, tile, overlap, tta, group):
    tc.check_equivariance(DEV, models[name], H, tile, overlap, tta, group)


def test_tta_none_is_the_default_path(models):
    tc.check_none_is_default(DEV, models["d3_convt"])


def test_tta_none_counters_and_accumulator(models):
    tc.check_none_counters(DEV, models["d3_convt"])


def test_tta_rejects_bad_arguments(models):
    tc.check_arguments(DEV, models["d3_convt"])
