"""CPU: hole filling of tracked masks - the host restatement (tests/fill_holes_ref.py) on planes whose answer is known by construction,
the public switch (SAM2AdapterConfig.fill_hole_area -> SAM2Adapter._video() -> VideoPredictor(fill_hole_area=...)) and the argument check."""
import numpy as np
import pytest

from tests.fill_holes_cases import constructed_cases, spiral
from tests.fill_holes_ref import FILL_VALUE, fill_holes_ref, random_planes

CASES = constructed_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_on_constructed_planes(case):
    name, x, max_area, expected = case
    before = x.copy()
    out, filled, kept = fill_holes_ref(x, max_area)
    assert np.array_equal(x.view(np.int32), before.view(np.int32))                   # the input is left alone
    assert out.dtype == np.float32 and np.array_equal(out.view(np.int32), expected.view(np.int32))
    changed = out.view(np.int32) != x.view(np.int32)
    assert (out[changed] == FILL_VALUE).all() and (filled > 0) == bool(changed.any())


def test_restatement_counts_components():
    x = np.ones((2, 9, 9), np.float32)
    x[0, 1, 1] = -1                      # 1 pixel
    x[0, 3:6, 3:6] = 0                   # 9 pixels
    x[1, 0, 0:8] = -2                    # 8 pixels
    x[1, 2, 8] = x[1, 3, 7] = -1         # 2 pixels, diagonal
    out, filled, kept = fill_holes_ref(x, 8)
    assert (filled, kept) == (3, 1)
    assert (out <= 0).sum() == 9 and (out == FILL_VALUE).sum() == 11
    assert fill_holes_ref(x, 1)[1:] == (1, 3) and fill_holes_ref(x, 9)[1:] == (4, 0)
    g, n = spiral()
    assert n > 1000 and fill_holes_ref(g, 8)[1:] == (0, 1)


def test_random_recipe_has_components_on_both_sides_of_the_threshold():
    """the recipe of the device test: its cases must fill and keep many components, or they would compare nothing"""
    for seed, shape, want in ((0, (3, 64, 64), (224, 54)), (1, (2, 37, 70), (98, 31)), (3, (4, 33, 130), (346, 90))):
        assert fill_holes_ref(random_planes(seed, shape), 8)[1:] == want


def test_config_field_and_resolution_order(monkeypatch):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    assert SAM2AdapterConfig().fill_hole_area is None
    assert SAM2AdapterConfig(fill_hole_area=8).fill_hole_area == 8
    built = []

    class FakePredictor:
        def __init__(self, engine, weights, num_maskmem=2, **kw):
            built.append((engine, weights, num_maskmem, kw))

    monkeypatch.setattr("saber_amd.adapters.sam2.automask.get_engine", lambda *a, **k: "engine")
    monkeypatch.setattr("saber_amd.pretrained_weights.load_weights", lambda *a, **k: {"w": 0})
    monkeypatch.setattr("saber_amd.adapters.sam2.video.VideoPredictor", FakePredictor)

    def resolved(cfg_value, env):
        if env is None:
            monkeypatch.delenv("SABER_AMD_FILL_HOLE_AREA", raising=False)
        else:
            monkeypatch.setenv("SABER_AMD_FILL_HOLE_AREA", env)
        SAM2Adapter(SAM2AdapterConfig(cfg="tiny", fill_hole_area=cfg_value), device="cuda:0")._video()
        engine, weights, num_maskmem, kw = built[-1]
        assert engine == "engine" and weights == {"w": 0} and num_maskmem == 2
        return kw["fill_hole_area"]

    assert resolved(None, None) == 0                     # the default route: off
    assert resolved(None, "") == 0
    assert resolved(None, "8") == 8                      # the environment, when the config does not say
    assert resolved(5, "8") == 5                         # the config wins
    assert resolved(0, "8") == 0                         # ... also when it says "off"
    assert resolved(8, None) == 8


def test_video_predictor_argument_check_needs_no_gpu():
    from saber_amd.adapters.sam2.video import VideoPredictor
    with pytest.raises(ValueError, match="fill_hole_area"):
        VideoPredictor(None, {}, fill_hole_area=-1)
