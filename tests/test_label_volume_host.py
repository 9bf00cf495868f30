"""CPU: the host side of the device-resident label volumes (saber_amd/utils/labelvol.py, csrc/labelvol.hip) - the presence filter's keep
table, the four C-ABI symbols in header, ctypes table and library, and the "no CPU fallback" errors of the opt-in routes."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("saber_k_paint_nearest_stack", "saber_k_relabel_frames", "saber_k_merge_max_u16", "saber_k_merge_class_conf")


def test_presence_keep_table_on_hand_made_bounds():
    from saber_amd.utils.labelvol import presence_keep_table
    bounds = np.array([[0.9, 0.1, 0.5],
                       [0.5, 0.5, 0.49999],
                       [0.0, 1.0, 0.50001],
                       [0.2, 0.3, 0.4]])
    t = presence_keep_table(bounds, 0.5)
    assert t.dtype == np.uint16 and t.shape == (4, 4)
    assert np.array_equal(t, np.array([[0, 1, 0, 3],          # 0.5 == threshold stays: the reference drops on `<`
                                       [0, 1, 2, 0],
                                       [0, 0, 2, 3],
                                       [0, 0, 0, 0]], dtype=np.uint16))
    assert (t[:, 0] == 0).all()
    # the table applied as a look-up is the reference's per-frame-and-object loop
    rng = np.random.default_rng(0)
    vol = rng.integers(0, 4, (4, 5, 6)).astype(np.uint16)
    ref = vol.copy()
    for z in range(4):
        for mi in range(3):
            if float(bounds[z, mi]) < 0.5:
                ref[z][ref[z] == mi + 1] = 0
    assert np.array_equal(np.take_along_axis(t, vol.reshape(4, -1).astype(np.int64), axis=1).reshape(vol.shape), ref)
    ident = presence_keep_table(bounds, -1.0)                   # nothing dropped: identity rows
    assert np.array_equal(ident, np.tile(np.arange(4, dtype=np.uint16), (4, 1)))
    assert presence_keep_table(np.zeros((3, 0)), 0.5).shape == (3, 1)
    with pytest.raises(ValueError):
        presence_keep_table(np.zeros(3), 0.5)


def test_symbols_in_header_ctypes_table_and_library(lib):
    from saber_amd import _lib
    txt = open(os.path.join(ROOT, "include", "saber_amd_kernels.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), f"{name} is not declared in include/saber_amd_kernels.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from the ctypes table"
        assert hasattr(lib, name), f"{name} is not exported by the library"


def test_device_routes_fail_loudly_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("has a GPU")
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.amg import cfgAMG
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    from saber_amd.segmenters.propagation import propagationSegmenter
    from saber_amd.segmenters.tomo import multiDepthTomoSegmenter
    seed = np.ones((8, 8), np.float32)
    for device in ("cuda:0", "cpu"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device=device).segment_volume(0, [seed], (3, 8, 8), device_volume=True)
    with pytest.raises(TypeError):                               # keyword-only
        SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cpu").segment_volume(0, [seed], (3, 8, 8), None, 0.5, None, True)
    vol = np.zeros((5, 16, 16), np.float32)
    cfg = SAM2AdapterConfig(cfg="tiny", amg_cfg=cfgAMG(npoints=8, crop_n_layers=0, sam2_cfg="small"), min_mask_area=50)
    ps = propagationSegmenter(deviceID=0, cfg=cfg, min_mask_area=50)
    assert ps.device_volumes is False
    ps.device_volumes = True
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ps.segment(vol, ini_depth=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ps.multiclass_segment(vol)
    md = multiDepthTomoSegmenter(deviceID=0, cfg=cfg, min_mask_area=50)
    md.device_volumes = True
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        md.segment(vol, thickness=2, num_slabs=3, delta_z=2)
