"""Whole-scene prediction on the gfx950 kernels: ``window_gather``, ``head_predict_accum``,
``scene_finalize`` and ``ScenePredictor`` (the bodies live in ``predict_cases.py`` and also
run on the CPU kernels, ``test_predict_cpu.py``)."""
import pytest

import predict_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def models():
    return {name: pc.make_model(name, DEV) for name in pc.MODELS}


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
