"""CPU: the classifier filter's new keywords (saber_amd/filters/masks.py) default to the host route and leave it unchanged; the device
route has no CPU fallback; the C-ABI symbol behind it is declared, bound and checks its arguments without a device."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from saber_amd.filters import masks as fm


def small_input():
    st = np.zeros((4, 9, 12), dtype=bool)
    st[0, 1:4, 1:5] = True
    st[1, 2:6, 3:8] = True                       # overlaps the first
    st[2, 7:9, 9:12] = True                      # apart, on the border
    st[3, 0, 11] = True                          # one pixel
    conf = np.array([0.75, 0.5625, 0.625, 0.875], dtype=np.float32)
    return [{"segmentation": m, "area": int(m.sum())} for m in st], conf


def test_keywords_exist_and_default_to_the_host_route():
    sig = inspect.signature(fm._consensus_based_resolution)
    assert list(sig.parameters)[:3] == ["image_shape", "masks", "confidences"]
    for name, default in (("device", None), ("masks_dev", None), ("min_area", 0)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default
    for fn, names in ((fm.convert_predictions_to_masks, ("device", "masks_dev")), (fm.apply_classifier, ("device",))):
        sig = inspect.signature(fn)
        for name in names:
            assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default is None
    assert list(inspect.signature(fm.apply_classifier).parameters)[:6] == ["image", "masks", "classifier", "desired_class", "min_mask_area", "batchsize"]
    assert list(inspect.signature(fm.convert_predictions_to_masks).parameters)[:4] == ["predictions", "masks", "desired_class", "min_mask_area"]


def test_host_route_output_is_unchanged():
    masks, conf = small_input()
    out = fm._consensus_based_resolution((9, 12), masks, conf)
    assert [m["area"] for m in out] == [1, 28, 6]
    assert [m["bbox"] for m in out] == [[11, 0, 0, 0], [1, 1, 6, 4], [9, 7, 2, 1]]
    assert [m["crop_box"] for m in out] == [[11, 0, 11, 0], [1, 1, 7, 5], [9, 7, 11, 8]]
    assert [m["point_coords"] for m in out] == [[[11, 0]], [[4, 3]], [[10, 7]]]
    assert list(out[0]) == ["segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"]
    # union of the two overlapping rectangles: 12 + 20 - 4 pixels; 4 of them average (0.75 + 0.5625) / 2
    assert out[1]["predicted_iou"] == out[1]["stability_score"] == pytest.approx((8 * 0.75 + 16 * 0.5625 + 4 * 0.65625) / 28, abs=1e-15)
    assert out[0]["predicted_iou"] == 0.875 and out[2]["predicted_iou"] == 0.625
    assert out[1]["segmentation"].dtype == np.bool_ and int(out[1]["segmentation"].sum()) == 28
    assert fm._consensus_based_resolution((9, 12), [], conf[:0]) == []
    assert [m["area"] for m in fm._consensus_based_resolution((9, 12), masks, conf, min_area=6)] == [28, 6]


def test_area_filter_handed_down_gives_the_same_list(monkeypatch):
    masks, conf = small_input()
    pred = np.stack([1.0 - conf, conf], axis=1).astype(np.float32)
    got = fm.convert_predictions_to_masks(pred, list(masks), 1, 5)
    real = fm._consensus_based_resolution
    seen = []

    def not_handed_down(image_shape, found, confidences, **kw):
        seen.append(kw.pop("min_area"))
        return real(image_shape, found, confidences, **kw)

    monkeypatch.setattr(fm, "_consensus_based_resolution", not_handed_down)
    want = fm.convert_predictions_to_masks(pred, list(masks), 1, 5)
    assert seen == [5]
    assert [m["area"] for m in got] == [m["area"] for m in want] == [6, 28]
    for a, b in zip(got, want):
        assert list(a) == list(b) and np.array_equal(a["segmentation"], b["segmentation"])
        assert all(a[key] == b[key] for key in a if key != "segmentation")
    assert fm.convert_predictions_to_masks(pred, list(masks), 1, 100) == []
    with pytest.raises(TypeError):
        fm.convert_predictions_to_masks(pred, list(masks), None, 5)


def test_device_route_has_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("has a GPU")
    masks, conf = small_input()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fm._consensus_based_resolution((9, 12), masks, conf, device=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fm._consensus_based_resolution((9, 12), masks, conf, device="cpu")
    with pytest.raises(ValueError):                     # argument checks come first
        fm._consensus_based_resolution((9, 12), masks, conf[:2], device=0)
    with pytest.raises(ValueError):
        fm._consensus_based_resolution((9, 13), masks, conf, device=0)
    pred = np.stack([1.0 - conf, conf], axis=1).astype(np.float32)

    class Stub:
        def batch_predict(self, image, segs, batch_size):
            return pred

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fm.apply_classifier(np.zeros((9, 12), np.float32), list(masks), Stub(), 1, 5, device=0)
    assert [m["area"] for m in fm.apply_classifier(np.zeros((9, 12), np.float32), list(masks), Stub(), 1, 5)] == [6, 28]


def test_symbol_is_bound_and_checks_its_arguments_without_a_device(lib):
    from saber_amd import _lib
    from saber_amd.engine import Engine
    assert "saber_consensus_components" in _lib.SIGNATURES and hasattr(lib, "saber_consensus_components")
    assert callable(Engine.consensus_components)
    assert Engine.CONSENSUS_ROW.itemsize == 32 and Engine.CONSENSUS_ROW.fields["avg_sum"][1] == 24
    n = C.c_int(3)
    assert lib.saber_consensus_components(None, None, 1, 1, 1, None, None, 1, 0, None, None, C.byref(n), None) == -1


def test_saber2d_switch_defaults_to_off():
    from saber_amd.segmenters.base import saber2D
    src = inspect.getsource(saber2D.__init__)
    assert "self.device_consensus = False" in src
