"""CPU: the mask generator's small-region step - the host restatement (tests/small_regions_ref.py) on stacks whose answer is known by
construction, the C-ABI symbols, the public switch (SAM2AdapterConfig.min_mask_region_area / SABER_AMD_MIN_MASK_REGION_AREA ->
build_amg -> EngineMaskGenerator -> Engine.amg_generate; segment_slice_to_plane) and the argument checks."""
import os
import re

import numpy as np
import pytest
import torch

from tests.small_regions_cases import constructed_cases
from tests.small_regions_ref import (RANDOM_CASES, clean_mask, nms_ref, pack_bits, random_case, small_regions_ref, tight_box, unpack_bits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = constructed_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_on_constructed_stacks(case):
    name, masks, A, exp, exp_changed = case
    assert masks.shape[1] <= 130 and masks.shape[2] <= 130
    ref = small_regions_ref(masks, A)
    assert np.array_equal(ref["masks"], exp), f"{name}: {int((ref['masks'] != exp).sum())} pixels differ"
    assert np.array_equal(ref["changed"], exp_changed)
    assert np.array_equal(ref["area"], exp.reshape(len(exp), -1).sum(1))
    assert np.array_equal(ref["boxes"], np.array([tight_box(m) for m in exp]))


def test_restatement_details():
    # the flag, not a pixel comparison: a single island below A keeps its pixels and is changed
    m = np.zeros((10, 33), bool)
    m[4, 30:33] = True
    new, h, i = clean_mask(m, 9)
    assert np.array_equal(new, m) and not h and i
    # a hole of exactly A stays, of A - 1 goes; the test is strict
    m = np.ones((12, 40), bool)
    m[3, 5:14] = False
    assert clean_mask(m, 9)[1:] == (False, False) and clean_mask(m, 10)[1:] == (True, False)
    # empty mask: box of zeros; NMS order: untouched first, ties keep ascending index, suppression needs IoU > T
    assert tight_box(np.zeros((4, 4), bool)) == [0, 0, 0, 0]
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [20, 20, 30, 30], [0, 0, 10, 9]])
    assert nms_ref(boxes, [0.0, 1.0, 0.0, 1.0], 0.7) == [1, 2]
    assert nms_ref(boxes, [0.0, 1.0, 0.0, 1.0], 1.0) == [1, 3, 0, 2]
    assert nms_ref(boxes, [1.0, 1.0, 1.0, 1.0], 0.95) == [0, 2, 3]
    # bit packing: bit b of word w = pixel 32 w + b, padding zero
    m = np.zeros((1, 1, 37), bool)
    m[0, 0, [0, 31, 32, 36]] = True
    w = pack_bits(m)
    assert w.shape == (1, 1, 2) and w[0, 0].tolist() == [0x80000001, 0x11] and np.array_equal(unpack_bits(w, 37), m)


@pytest.mark.parametrize("case", RANDOM_CASES, ids=[str(c) for c in RANDOM_CASES])
def test_random_stacks_are_not_vacuous(case):
    masks, ref = random_case(case)
    n = case[1]
    assert int(ref["changed"].sum()) >= n // 2 and n - len(ref["keep"]) >= 2 and ref["keep"] != sorted(ref["keep"])


def test_symbols_in_header_table_and_library(lib):
    from saber_amd import _lib
    kern = open(os.path.join(ROOT, "include", "saber_amd_kernels.h")).read()
    eng = open(os.path.join(ROOT, "include", "saber_amd.h")).read()
    for name, txt in (("saber_k_mask_small_regions", kern), ("saber_k_mask_small_regions_bytes", kern), ("saber_amg_postprocess_small_regions", eng)):
        assert re.search(r"\b" + name + r"\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    per = lib.saber_k_mask_small_regions_bytes(1024, 1024)
    assert 1024 * 1024 * 8 + 1024 * 32 * 4 <= per <= 1024 * 1024 * 8 + 1024 * 32 * 4 + 1024
    assert lib.saber_k_mask_small_regions_bytes(0, 5) == 0
    # argument errors are found before anything touches a device
    assert lib.saber_k_mask_small_regions(None, 1, 8, 8, 9, None, None, None, None, None, 0, None) == -1
    assert lib.saber_k_last_error().decode().startswith("mask_small_regions:")
    assert "min_mask_region_area" not in [f[0] for f in _lib.AmgParams._fields_]


def test_config_and_environment(monkeypatch):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2 import SAM2Adapter
    import saber_amd.adapters.sam2.predictor as pred
    assert SAM2AdapterConfig().min_mask_region_area is None
    assert SAM2AdapterConfig(min_mask_region_area=25).min_mask_region_area == 25
    with pytest.raises(ValueError, match="min_mask_region_area"):
        SAM2AdapterConfig(min_mask_region_area=-1)
    seen = {}

    def fake_build_amg(amg, min_mask_area, device="cuda", checkpoint=None, **kw):
        seen.update(kw)
        return object()

    monkeypatch.setattr(pred, "build_amg", fake_build_amg)

    def built_with(cfg_value, env):
        seen.clear()
        if env is None:
            monkeypatch.delenv("SABER_AMD_MIN_MASK_REGION_AREA", raising=False)
        else:
            monkeypatch.setenv("SABER_AMD_MIN_MASK_REGION_AREA", env)
        SAM2Adapter(SAM2AdapterConfig(cfg="tiny", min_mask_region_area=cfg_value), device="cuda:0")._generator()
        return seen["min_mask_region_area"]

    assert built_with(None, None) == 0                              # off by default
    assert built_with(None, "25") == 25                             # the environment, when the config does not say
    assert built_with(10, "25") == 10                               # the config wins
    assert built_with(0, "25") == 0                                 # also when it says off
    with pytest.raises(ValueError, match="min_mask_region_area"):
        built_with(None, "-3")


class StubEngine:
    """records the amg_generate calls it gets; returns no masks"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def prepare(self, x):
        return x.to(torch.float32)

    def amg_generate(self, img, params, **kw):
        self.calls.append(kw)
        return torch.zeros((0, img.shape[0], (img.shape[1] + 31) // 32), dtype=torch.int32), []


def test_keyword_reaches_the_engine(monkeypatch):
    from saber_amd.adapters.sam2 import automask
    from saber_amd.segmenters.slice_driver import segment_slice_to_plane
    img = np.zeros((8, 40), np.float32)
    # EngineMaskGenerator
    eng = StubEngine()
    automask.EngineMaskGenerator(eng, automask.get_default(), min_mask_region_area=25).generate_device(img)
    assert eng.calls == [{"max_masks": 2048, "min_mask_region_area": 25}]
    eng = StubEngine()
    gen = automask.EngineMaskGenerator(eng, automask.get_default())
    assert gen.min_mask_region_area == 0
    gen.generate_device(img)
    assert eng.calls == [{"max_masks": 2048}]                       # 0: the step is not asked for
    with pytest.raises(ValueError, match="min_mask_region_area"):
        automask.EngineMaskGenerator(eng, automask.get_default(), min_mask_region_area=-1)
    # build_amg
    eng = StubEngine()
    monkeypatch.setattr(automask, "get_engine", lambda *a, **k: eng)
    g = automask.build_amg(dict(automask.get_default(), sam2_cfg="tiny"), 50, min_mask_region_area=7)
    assert g.base_generator.min_mask_region_area == 7
    g.base_generator.generate_device(img)
    assert eng.calls == [{"max_masks": 2048, "min_mask_region_area": 7}]
    assert automask.build_amg(dict(automask.get_default(), sam2_cfg="tiny"), 50).base_generator.min_mask_region_area == 0
    with pytest.raises(ValueError, match="min_mask_region_area"):
        automask.build_amg(dict(automask.get_default(), sam2_cfg="tiny"), 50, min_mask_region_area=-2)
    # segment_slice_to_plane
    eng = StubEngine()
    plane, n = segment_slice_to_plane(eng, torch.zeros((8, 40)), None, min_mask_region_area=12)
    assert n == 0 and eng.calls == [{"max_masks": 2048, "min_mask_region_area": 12}]
    eng = StubEngine()
    segment_slice_to_plane(eng, torch.zeros((8, 40)), None)
    assert eng.calls == [{"max_masks": 2048}]


def test_engine_methods_fail_loudly_without_device():
    if torch.cuda.is_available():
        pytest.skip("has a GPU")
    from saber_amd.engine import Engine
    eng = Engine.__new__(Engine)                                    # no handle can be made without a device
    eng.h = None
    bits = torch.zeros((1, 4, 1), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.remove_small_regions(bits, 8, 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.postprocess_small_regions(bits, [None], 4, 8, 9, 0.7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Engine.bare(0)


def test_amg_generate_keyword_checks():
    """the keyword is validated, and 0 never reaches the step (the call below fails before any engine state is read)"""
    from saber_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.h = None
    with pytest.raises(ValueError, match="min_mask_region_area"):
        eng.amg_generate(None, None, min_mask_region_area=-1)
    called = []
    eng.postprocess_small_regions = lambda *a, **k: called.append(a) or ("bits", "meta")
    eng.amg_generate = lambda img, params, max_masks=1024, **kw: (called.append(("inner", kw)) or (torch.zeros((0, 4, 1), dtype=torch.int32), []))
    p = type("P", (), {"box_nms_thresh": 0.7, "crop_nms_thresh": 0.8})()
    assert Engine.amg_generate(eng, torch.zeros((4, 8)), p, min_mask_region_area=5) == ("bits", "meta")
    assert called[0] == ("inner", {}) and called[1][2:] == (4, 8, 5, 0.8)                  # T = max(box_nms_thresh, crop_nms_thresh)
