"""CPU: the clean-up of the low-resolution mask logits (upstream's max_hole_area / max_sprinkle_area) - the scipy restatement on planes
whose answer is known by construction, the C-ABI symbols, the refusals that need no device, and the public switches
(Engine.amg_generate / EngineMaskGenerator / build_amg / segment_slice_to_plane keywords, SAM2AdapterConfig, SABER_AMD_MAX_HOLE_AREA /
SABER_AMD_MAX_SPRINKLE_AREA)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import lowres_cleanup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HI, LO = np.float32(10.0), np.float32(-10.0)


# ------------------------------------------------------------------------------------------------ the restatement
def test_fill_values():
    assert R.fill_values(0.0) == (HI, LO)
    assert R.fill_values(0.5) == (np.float32(10.5), np.float32(-9.5))
    t = np.float32(0.1)
    assert R.fill_values(0.1) == (np.float32(np.float64(t) + 10.0), np.float32(np.float64(t) - 10.0))


def test_boundary_is_at_most():
    x = R.exact_sizes(17, 33, 8)
    for h, s in ((8, 0), (0, 8), (8, 8), (9, 9), (7, 7)):
        out = R.clean_lowres_ref(x, 0.0, h, s)[0]
        exp = x[0].copy()
        if h >= 8:
            exp[2, 2:10] = HI; exp[0, 16:24] = HI                  # exactly 8: filled, inside and on the border
        if h >= 9:
            exp[4, 2:11] = HI; exp[16, 16:25] = HI                 # 9: only from 9 on
        if h >= 3:
            exp[7:10, 32] = HI; exp[16, 0] = HI                    # pockets on the border and in the corner are holes
        if s >= 8:
            exp[8, 2:10] = LO
        if s >= 9:
            exp[10, 2:11] = LO
        assert np.array_equal(R.bits(out), R.bits(exp)), (h, s)
    # the block of 109 around the two pieces stays below its size and goes at it
    assert (R.clean_lowres_ref(x, 0.0, 108, 0)[0, 6:15, 0:14] == HI).sum() == 0
    assert (R.clean_lowres_ref(x, 0.0, 109, 0)[0, 6:15, 0:14] == HI).sum() == 109


def test_hole_inside_a_sprinkle():
    x = R.hole_in_sprinkle()
    out = R.clean_lowres_ref(x, 0.0, 30, 30)[0]
    exp = x[0].copy()
    exp[4:9, 6:11] = LO                                            # the island of 24 goes ...
    exp[6, 8] = HI                                                 # ... and its hole is filled all the same: both labellings are of the original plane
    assert np.array_equal(R.bits(out), R.bits(exp))
    assert np.array_equal(R.bits(R.clean_lowres_ref(x, 0.0, 1, 23)[0, 4:9, 6:11]), R.bits(np.where(x[0, 4:9, 6:11] > 0, x[0, 4:9, 6:11], HI)))   # 24 > 23
    only_s = R.clean_lowres_ref(x, 0.0, 0, 24)[0]
    assert only_s[6, 8] == np.float32(-0.5) and (only_s[4:9, 6:11] == LO).sum() == 24
    assert np.array_equal(R.bits(R.clean_lowres_ref(x, 0.0, 0, 0)), R.bits(x))


def test_special_values_and_threshold():
    x = R.special_values()
    out = R.clean_lowres_ref(x, 0.0, 8, 8)[0]
    assert out[1, 3] == HI and out[1, 7] == HI                     # both zeros are background at t = 0
    assert (out[3, 2:10] == HI).all()                              # a run of 8 zeros of both signs is ONE component
    assert (out[5, 2:10] == HI).all() and (out[5, 11:19] == HI).all() and np.isnan(out[5, 10])       # NaN separates, and stays
    assert R.bits(out)[7, 4] == R.bits(x)[0, 7, 4] and R.bits(out)[5, 10] == R.bits(x)[0, 5, 10]     # NaN bits (sign included) kept
    assert out[9, 5] == np.float32(1e-45) and out[9, 7] == HI      # denormals have a sign: one belongs to the foreground around it, one is a hole of 1
    assert out[12, 21] == LO and np.isnan(out[11:14, 20:23]).sum() == 8
    assert (out[14, 2:4] == HI).all() and (out[14, 5:8] == HI).all() and np.isnan(out[14, 4])
    out7 = R.clean_lowres_ref(x, 0.0, 7, 0)[0]
    assert (out7[3, 2:10] == x[0, 3, 2:10]).all() and np.signbit(out7[3, 6])                          # 8 > 7: kept, -0.0 still -0.0
    y = R.threshold_half()
    out = R.clean_lowres_ref(y, 0.5, 4, 3)[0]
    assert (out[2, 2:6] == np.float32(10.5)).all() and out[2, 6] == y[0, 2, 6] and (out[2, 7:10] == np.float32(10.5)).all()
    assert (out[8, 12:15] == np.float32(-9.5)).all() and (out[10, 12:15] == np.float32(0.5)).all()
    z = R.adjacent_planes()
    assert (R.clean_lowres_ref(z, 0.0, 0, 5) > 0).sum() == 0       # six pieces of 5, none of 10
    assert np.array_equal(R.bits(R.clean_lowres_ref(z, 0.0, 0, 4)), R.bits(z))


def test_whole_plane_components_and_shapes():
    for sign in (1.0, -1.0):
        x = R.distinct(1, 256, 256, sign=sign)
        assert np.array_equal(R.bits(R.clean_lowres_ref(x, 0.0, 65535, 65535)), R.bits(x))           # 65 536 > 65 535
        y = R.distinct(1, 255, 257, sign=sign)
        assert (R.clean_lowres_ref(y, 0.0, 65535, 65535) == (LO if sign > 0 else HI)).all()
    cb = R.checkerboard(256, 256)
    out = R.clean_lowres_ref(cb, 0.0, 32768, 32767)                # each polarity is ONE diagonal-connected component of 32 768
    assert (out[cb <= 0] == HI).all() and np.array_equal(out[cb > 0], cb[cb > 0])
    g, n = R.spiral(64, 100)
    assert n > 1000
    assert np.array_equal(R.clean_lowres_ref(g, 0.0, n - 1, 0), g) and (R.clean_lowres_ref(g, 0.0, n, 0) > 0).all()
    names = [c[0] for c in R.kernel_cases()]
    assert len(set(names)) == len(names) and all(any(f"{H}x{W}" in m for m in names) for (H, W) in R.SHAPES)


# ------------------------------------------------------------------------------------------------ the library
def test_symbols_and_refusals(lib):
    from saber_amd import _lib
    kern = open(os.path.join(ROOT, "include", "saber_amd_kernels.h")).read()
    eng = open(os.path.join(ROOT, "include", "saber_amd.h")).read()
    for name, txt in (("saber_k_clean_lowres", kern), ("saber_engine_set_lowres_cleanup", eng)):
        assert re.search(r"\b" + name + r"\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    for f in ("max_hole_area", "max_sprinkle_area"):
        assert f not in [x[0] for x in _lib.AmgParams._fields_]    # saber_amg_params does not grow (tests/test_abi.py pins its size)
    # argument errors are found before anything touches a device; the pointer below is never read
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    bad = [(None, 1, 8, 8, 1, 1), (p, -1, 8, 8, 1, 1), (p, 1, 0, 8, 1, 1), (p, 1, 8, 0, 1, 1), (p, 1, 257, 256, 1, 1), (p, 1, 1, 65537, 1, 1),
           (p, 1, 8, 8, -1, 1), (p, 1, 8, 8, 1, -1), (p, 1, 8, 8, 65536, 1), (p, 1, 8, 8, 1, 65536)]
    for planes, n, H, W, h, s in bad:
        assert lib.saber_k_clean_lowres(planes, None, None, n, H, W, 0.0, h, s, None) == -1, (n, H, W, h, s)
        assert lib.saber_k_last_error().decode().startswith("clean_lowres:")
    assert not buf.any()
    assert lib.saber_engine_set_lowres_cleanup(None, 1, 1) == -1


# ------------------------------------------------------------------------------------------------ the switches
def test_config_and_environment(monkeypatch):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2 import SAM2Adapter
    import saber_amd.adapters.sam2.predictor as pred
    c = SAM2AdapterConfig()
    assert c.max_hole_area is None and c.max_sprinkle_area is None and c.min_mask_region_area is None
    assert SAM2AdapterConfig(max_hole_area=25, max_sprinkle_area=7).max_sprinkle_area == 7
    for bad in (dict(max_hole_area=-1), dict(max_sprinkle_area=-1), dict(max_hole_area=65536), dict(max_sprinkle_area=70000)):
        with pytest.raises(ValueError, match="max_(hole|sprinkle)_area"):
            SAM2AdapterConfig(**bad)
    seen = {}

    def fake_build_amg(amg, min_mask_area, device="cuda", checkpoint=None, **kw):
        seen.update(kw)
        return object()

    monkeypatch.setattr(pred, "build_amg", fake_build_amg)

    def built_with(cfg, env):
        seen.clear()
        for var, v in zip(("SABER_AMD_MAX_HOLE_AREA", "SABER_AMD_MAX_SPRINKLE_AREA"), env):
            if v is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, v)
        SAM2Adapter(SAM2AdapterConfig(cfg="tiny", max_hole_area=cfg[0], max_sprinkle_area=cfg[1]), device="cuda:0")._generator()
        return seen["max_hole_area"], seen["max_sprinkle_area"], seen["min_mask_region_area"]

    monkeypatch.delenv("SABER_AMD_MIN_MASK_REGION_AREA", raising=False)
    assert built_with((None, None), (None, None)) == (0, 0, 0)      # off by default
    assert built_with((None, None), ("25", "9")) == (25, 9, 0)      # the environment, when the config does not say; min_mask_region_area is its own option
    assert built_with((10, None), ("25", "9")) == (10, 9, 0)        # the config wins, field by field
    assert built_with((0, 0), ("25", "9")) == (0, 0, 0)             # also when it says off
    assert built_with((None, None), ("", None)) == (0, 0, 0)
    for env in (("-3", None), (None, "65536"), ("many", None)):
        with pytest.raises(ValueError, match="SABER_AMD_MAX_(HOLE|SPRINKLE)_AREA"):
            built_with((None, None), env)
    monkeypatch.setenv("SABER_AMD_MIN_MASK_REGION_AREA", "25")      # ... and the other way round
    assert built_with((None, None), (None, None)) == (0, 0, 25)


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


def test_keywords_reach_the_engine(monkeypatch):
    from saber_amd.adapters.sam2 import automask
    from saber_amd.segmenters.slice_driver import segment_slice_to_plane
    img = np.zeros((8, 40), np.float32)
    eng = StubEngine()
    gen = automask.EngineMaskGenerator(eng, automask.get_default(), max_hole_area=25, max_sprinkle_area=9)
    assert (gen.max_hole_area, gen.max_sprinkle_area, gen.min_mask_region_area) == (25, 9, 0)
    gen.generate_device(img)
    assert eng.calls == [{"max_masks": 2048, "max_hole_area": 25, "max_sprinkle_area": 9}]
    eng = StubEngine()
    automask.EngineMaskGenerator(eng, automask.get_default(), min_mask_region_area=25, max_hole_area=25, max_sprinkle_area=25).generate_device(img)
    assert eng.calls == [{"max_masks": 2048, "min_mask_region_area": 25, "max_hole_area": 25, "max_sprinkle_area": 25}]      # an upstream build with its extension
    eng = StubEngine()
    automask.EngineMaskGenerator(eng, automask.get_default(), max_sprinkle_area=3).generate_device(img)
    assert eng.calls == [{"max_masks": 2048, "max_hole_area": 0, "max_sprinkle_area": 3}]
    eng = StubEngine()
    gen = automask.EngineMaskGenerator(eng, automask.get_default())
    assert (gen.max_hole_area, gen.max_sprinkle_area) == (0, 0)
    gen.generate_device(img)
    assert eng.calls == [{"max_masks": 2048}]                       # 0 / 0: the step is not asked for
    for bad in (dict(max_hole_area=-1), dict(max_sprinkle_area=65536), dict(max_hole_area=2.5)):
        with pytest.raises(ValueError, match="max_(hole|sprinkle)_area"):
            automask.EngineMaskGenerator(eng, automask.get_default(), **bad)
        with pytest.raises(ValueError, match="max_(hole|sprinkle)_area"):
            automask.build_amg(dict(automask.get_default(), sam2_cfg="tiny"), 50, **bad)
    # build_amg
    eng = StubEngine()
    monkeypatch.setattr(automask, "get_engine", lambda *a, **k: eng)
    g = automask.build_amg(dict(automask.get_default(), sam2_cfg="tiny"), 50, max_hole_area=7, max_sprinkle_area=8)
    assert (g.base_generator.max_hole_area, g.base_generator.max_sprinkle_area) == (7, 8)
    g.base_generator.generate_device(img)
    assert eng.calls == [{"max_masks": 2048, "max_hole_area": 7, "max_sprinkle_area": 8}]
    assert automask.build_amg(dict(automask.get_default(), sam2_cfg="tiny"), 50).base_generator.max_hole_area == 0
    # segment_slice_to_plane
    eng = StubEngine()
    plane, n = segment_slice_to_plane(eng, torch.zeros((8, 40)), None, max_hole_area=12, max_sprinkle_area=0)
    assert n == 0 and eng.calls == [{"max_masks": 2048, "max_hole_area": 12, "max_sprinkle_area": 0}]
    eng = StubEngine()
    segment_slice_to_plane(eng, torch.zeros((8, 40)), None, min_mask_region_area=5, max_sprinkle_area=4)
    assert eng.calls == [{"max_masks": 2048, "min_mask_region_area": 5, "max_hole_area": 0, "max_sprinkle_area": 4}]


def test_amg_generate_keywords():
    """the keywords are validated; non-zero ones are set on the handle for the call and the handle's own setting is back afterwards"""
    from saber_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.h = None
    for bad in (dict(max_hole_area=-1), dict(max_sprinkle_area=65536), dict(max_hole_area=True)):
        with pytest.raises(ValueError, match="max_(hole|sprinkle)_area"):
            eng.amg_generate(None, None, **bad)
    log = []
    eng.set_lowres_cleanup = lambda h, s: log.append(("set", h, s))
    eng.amg_generate = lambda img, params, max_masks=1024, **kw: (log.append(("inner", max_masks, kw)) or ("bits", "meta"))
    assert Engine.amg_generate(eng, torch.zeros((4, 8)), None, max_masks=7, max_hole_area=25, max_sprinkle_area=9, min_mask_region_area=3) == ("bits", "meta")
    assert log == [("set", 25, 9), ("inner", 7, {"min_mask_region_area": 3}), ("set", 0, 0)]
    log.clear()
    eng._lowres_cleanup = (4, 5)                                    # what set_lowres_cleanup left on the handle
    Engine.amg_generate(eng, torch.zeros((4, 8)), None, max_sprinkle_area=2)
    assert log == [("set", 0, 2), ("inner", 1024, {"min_mask_region_area": 0}), ("set", 4, 5)]


def test_clean_lowres_wants_device_planes():
    """host planes never reach the library: without a device there is no fallback, with one the tensor is refused"""
    from saber_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.h = None
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="device tensor"):
            eng.clean_lowres(torch.zeros((1, 4, 4)), 1, 1)
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            eng.clean_lowres(torch.zeros((1, 4, 4)), 1, 1)
