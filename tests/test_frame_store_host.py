"""The frame-feature store of the video path, host side (saber_amd/adapters/sam2/video.py: plan_window, frame_store_rows,
frame_store_budget; SAM2AdapterConfig.frame_store_gb -> SAM2Adapter._video() -> VideoPredictor(frame_store_gb=...)).  No GPU."""
import inspect

import pytest

from saber_amd.adapters.sam2.video import (FRAME_STORE_BYTES, FRAME_STORE_SIZES, VideoPredictor, frame_store_budget, frame_store_rows,
                                           plan_window)


def test_planner_all_frames_stored():
    assert plan_window(2, 6, {2: 0, 3: 1, 4: 2, 5: 3}, 0) == ([], [], True)          # nothing to encode: served even with no row left
    assert plan_window(2, 6, set(range(10)), 5) == ([], [], True)


def test_planner_none_stored_with_rows_free():
    assert plan_window(5, 9, {}, 10) == ([5, 6, 7, 8], [5, 6, 7, 8], True)
    assert plan_window(5, 9, set(), 4) == ([5, 6, 7, 8], [5, 6, 7, 8], True)          # exactly enough


def test_planner_partly_stored_window():
    # frame 5 was stored by a forward window; the reverse window [2, 6) misses three frames that are not a prefix of the store's order
    assert plan_window(2, 6, {5: 0, 6: 1, 7: 2, 8: 3, 9: 4}, 5) == ([2, 3, 4], [2, 3, 4], True)
    # a hole in the middle: the missing frames are not contiguous
    assert plan_window(0, 4, {1: 0, 3: 1}, 2) == ([0, 2], [0, 2], True)


def test_planner_rows_exhausted_falls_back_and_stores_nothing():
    assert plan_window(5, 9, {}, 3) == ([5, 6, 7, 8], [], False)
    assert plan_window(2, 6, {5: 0}, 2) == ([2, 3, 4], [], False)
    assert plan_window(0, 1, {}, 0) == ([0], [], False)
    assert plan_window(9, 10, {5: 0, 6: 1}, 1) == ([9], [9], True)                    # a later, shorter window still gets the last row


def test_planner_reverse_window_at_the_start_of_the_volume():
    # _frame(t=1, reverse=True) with windows of 4: [max(0, 1 - 3), 2) = [0, 2)
    assert plan_window(0, 2, {2: 0, 3: 1, 4: 2, 5: 3}, 6) == ([0, 1], [0, 1], True)
    assert plan_window(0, 1, {0: 0}, 0) == ([], [], True)


def test_planner_is_pure():
    stored = {1: 0}
    plan_window(0, 3, stored, 5)
    assert stored == {1: 0}


def test_row_arithmetic():
    assert FRAME_STORE_SIZES == (4096 * 256, 16384 * 64, 65536 * 32)
    assert FRAME_STORE_BYTES == 16_777_216
    assert frame_store_rows(2 ** 30, 1000) == 64
    assert frame_store_rows(2 ** 30, 10) == 10                    # capped at the volume's frames
    assert frame_store_rows(FRAME_STORE_BYTES - 1, 10) == 0       # whole frames only
    assert frame_store_rows(3 * FRAME_STORE_BYTES, 10) == 3
    assert frame_store_rows(0, 10) == 0
    assert frame_store_budget(1) == 2 ** 30
    assert frame_store_rows(frame_store_budget(3 * 16 / 1024), 10) == 3


def test_budget_reads_the_environment_only_without_an_argument(monkeypatch):
    monkeypatch.delenv("SABER_AMD_VIDEO_STORE_GB", raising=False)
    assert frame_store_budget(None) == 0                          # the default route: off
    monkeypatch.setenv("SABER_AMD_VIDEO_STORE_GB", "")
    assert frame_store_budget(None) == 0
    monkeypatch.setenv("SABER_AMD_VIDEO_STORE_GB", "2")
    assert frame_store_budget(None) == 2 * 2 ** 30
    assert frame_store_budget(0.5) == 2 ** 29                     # the argument wins
    assert frame_store_budget(0) == 0                             # ... also when it says "off"
    monkeypatch.setenv("SABER_AMD_VIDEO_STORE_GB", "-1")
    with pytest.raises(ValueError, match="frame_store_gb"):
        frame_store_budget(None)
    assert frame_store_budget(1) == 2 ** 30


def test_negative_budget_is_refused_without_a_gpu():
    with pytest.raises(ValueError, match="frame_store_gb"):
        frame_store_budget(-0.5)
    with pytest.raises(ValueError, match="frame_store_gb"):
        frame_store_budget(float("nan"))
    with pytest.raises(ValueError, match="frame_store_gb"):
        VideoPredictor(None, {}, frame_store_gb=-1)
    p = inspect.signature(VideoPredictor.__init__).parameters["frame_store_gb"]
    assert p.default is None


def test_config_field_reaches_the_video_predictor(monkeypatch):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    assert SAM2AdapterConfig().frame_store_gb is None
    assert SAM2AdapterConfig(frame_store_gb=1).frame_store_gb == 1
    with pytest.raises(ValueError, match="frame_store_gb"):
        SAM2AdapterConfig(frame_store_gb=-1)
    built = []

    class FakePredictor:
        def __init__(self, engine, weights, num_maskmem=2, **kw):
            built.append(kw)

    monkeypatch.setattr("saber_amd.adapters.sam2.automask.get_engine", lambda *a, **k: "engine")
    monkeypatch.setattr("saber_amd.pretrained_weights.load_weights", lambda *a, **k: {"w": 0})
    monkeypatch.setattr("saber_amd.adapters.sam2.video.VideoPredictor", FakePredictor)
    monkeypatch.setenv("SABER_AMD_VIDEO_STORE_GB", "4")
    for value in (None, 0, 0.25, 1):
        SAM2Adapter(SAM2AdapterConfig(cfg="tiny", frame_store_gb=value), device="cuda:0")._video()
        assert built[-1]["frame_store_gb"] == value and (value is None) == (built[-1]["frame_store_gb"] is None)
