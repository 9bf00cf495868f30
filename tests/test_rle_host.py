"""CPU: the mask generator's run-length output - the host restatement (tests/rle_ref.py) against transformers' SAM2 helpers on the
constructed stacks, the host helpers of saber_amd/adapters/sam2/rle.py, the C-ABI symbols, the argument checks and the public switch
(EngineMaskGenerator / build_amg output_mode).  Every comparison is exact equality."""
import ast
import importlib
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import rle_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HF = []


def _hf_rle_functions():
    """transformers.models.sam2.image_processing_sam2._mask_to_rle / _rle_to_mask.  Where the module does not import (it wants torchvision
    for its NMS) the two definitions, which need torch only, are compiled straight from the installed file, as
    tests/test_oracle_amg_vs_transformers.py does; without the file the comparison is skipped."""
    if not _HF:
        try:
            hf = importlib.import_module("transformers.models.sam2.image_processing_sam2")
            _HF.append((hf._mask_to_rle, hf._rle_to_mask))
        except Exception:                                            # noqa: BLE001 - any failure of the optional import
            spec = importlib.util.find_spec("transformers")
            path = spec and os.path.join(list(spec.submodule_search_locations)[0], "models", "sam2", "image_processing_sam2.py")
            if not path or not os.path.exists(path):
                _HF.append(None)
            else:
                want = {"_mask_to_rle", "_rle_to_mask"}
                body = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in want]
                if {n.name for n in body} != want:
                    _HF.append(None)
                else:
                    ns = {"torch": torch, "Any": object}
                    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
                    _HF.append((ns["_mask_to_rle"], ns["_rle_to_mask"]))
    if _HF[0] is None:
        pytest.skip("this transformers build has no SAM2 RLE helpers")
    return _HF[0]


@pytest.mark.parametrize("size", rle_ref.SIZES, ids=[f"{h}x{w}" for h, w in rle_ref.SIZES])
def test_restatement_against_transformers(size):
    to_rle, to_mask = _hf_rle_functions()
    H, W = size
    names, masks = rle_ref.constructed_stack(H, W)
    theirs = to_rle(torch.from_numpy(masks))
    for name, m, t in zip(names, masks, theirs):
        mine = rle_ref.encode(m)
        assert t["size"] == [H, W] and [int(c) for c in t["counts"]] == mine, name
        assert np.array_equal(to_mask({"size": [H, W], "counts": mine}).numpy(), m), name


@pytest.mark.parametrize("size", rle_ref.SIZES, ids=[f"{h}x{w}" for h, w in rle_ref.SIZES])
def test_restatement_properties(size):
    H, W = size
    names, masks = rle_ref.constructed_stack(H, W)
    assert names[:3] == ["checkerboard 0", "empty", "checkerboard 1"] and not masks[1].any()       # an empty mask between two dense ones
    for name, m in zip(names, masks):
        c = rle_ref.encode(m)
        assert sum(c) == H * W and all(v > 0 for v in c[1:]) and (c[0] == 0) == bool(m[0, 0]), name
        assert sum(c[1::2]) == int(m.sum()), name
        assert np.array_equal(rle_ref.decode(c, H, W), m), name
        assert np.array_equal(rle_ref.unpack_bits(rle_ref.pack_bits(masks, padding=True), W), masks)
    assert rle_ref.encode(np.zeros((3, 2), bool)) == [6] and rle_ref.encode(np.ones((3, 2), bool)) == [0, 6]
    m = np.zeros((3, 2), bool)
    m[2, 0] = m[0, 1] = True                                         # one run across the column border
    assert rle_ref.encode(m) == [2, 2, 2]
    # over-long and short counts: clamped at H W, zero behind the last run
    assert rle_ref.decode([1, 100], 3, 2).reshape(-1).tolist() == [False, True, True, True, True, True]
    assert rle_ref.decode([0, 2], 3, 2).T.reshape(-1).tolist() == [True, True, False, False, False, False]


def test_host_helpers():
    from saber_amd.adapters.sam2 import rle
    H, W = 65, 33
    names, masks = rle_ref.constructed_stack(H, W)
    for name, m in zip(names, masks):
        d = {"size": [H, W], "counts": rle_ref.encode(m)}
        back = rle.rle_to_mask(d)
        assert back.dtype == np.bool_ and back.shape == (H, W) and np.array_equal(back, m), name
        assert rle.area_from_rle(d) == int(m.sum()), name
    for bad in ({"size": [3, 2], "counts": [5]}, {"size": [3, 2], "counts": [3, 4]}, {"size": [3, 2], "counts": []}, {"size": [0, 2], "counts": [0]},
                {"size": [3, 2], "counts": [8, -2]}):
        with pytest.raises(ValueError, match="uncompressed RLE"):
            rle.rle_to_mask(bad)
    assert rle.OUTPUT_MODES == ("binary_mask", "uncompressed_rle", "coco_rle")


class UploadEngine:
    """an engine whose rle_decode records what reaches it (CPU tensors)"""
    device = torch.device("cpu")

    def rle_decode(self, counts, offsets, H, W):
        self.seen = (counts.clone(), offsets.clone(), H, W)
        return "bits"


def test_rles_to_device_validates_and_uploads():
    from saber_amd.adapters.sam2 import rle
    H, W = 5, 3
    a, b = np.zeros((H, W), bool), np.ones((H, W), bool)
    a[1:3, 1] = True
    eng = UploadEngine()
    ds = [{"size": [H, W], "counts": rle_ref.encode(m)} for m in (a, b, a)]
    assert rle.rles_to_device(ds, eng) == "bits"
    counts, offsets, h, w = eng.seen
    assert (h, w) == (H, W) and offsets.dtype == torch.int64 and offsets.tolist() == [0, 3, 5, 8]
    assert counts.dtype == torch.int32 and counts.tolist() == [6, 2, 7, 0, 15, 6, 2, 7]
    with pytest.raises(ValueError, match="no masks"):
        rle.rles_to_device([], eng)
    with pytest.raises(ValueError, match="size"):
        rle.rles_to_device([ds[0], {"size": [W, H], "counts": [15]}], eng)
    with pytest.raises(ValueError, match="summing to 14"):
        rle.rles_to_device([ds[0], {"size": [H, W], "counts": [14]}], eng)
    with pytest.raises(ValueError, match="2\\^31"):
        rle.rles_to_device([{"size": [1 << 16, 1 << 15], "counts": [1 << 31]}], eng)


def test_rle_dicts_splits_one_download():
    from saber_amd.adapters.sam2 import rle
    counts = torch.tensor([6, 2, 7, 0, 15], dtype=torch.int32)
    offsets = torch.tensor([0, 3, 5], dtype=torch.int64)
    out = rle.rle_dicts(counts, offsets, 5, 3)
    assert out == [{"size": [5, 3], "counts": [6, 2, 7]}, {"size": [5, 3], "counts": [0, 15]}]
    assert all(type(v) is int for d in out for v in d["counts"] + d["size"])
    assert rle.rle_dicts(counts[:0], offsets[:1], 5, 3) == []
    with pytest.raises(ValueError, match="offsets"):
        rle.rle_dicts(counts, torch.tensor([0, 3, 4], dtype=torch.int64), 5, 3)


def test_coco_rle_needs_pycocotools(monkeypatch):
    from saber_amd.adapters.sam2 import automask, rle
    monkeypatch.setitem(sys.modules, "pycocotools", None)            # "not installed", whether it is or not
    with pytest.raises(ImportError, match="pycocotools"):
        rle.coco_encode_rle({"size": [3, 2], "counts": [6]})
    with pytest.raises(ImportError, match="pycocotools"):
        automask.EngineMaskGenerator(object(), automask.get_default(), output_mode="coco_rle")


def test_symbols_in_header_table_and_library(lib):
    from saber_amd import _lib
    kern = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "saber_amd_kernels.h")).read(), flags=re.S)
    for name in ("saber_k_rle_workspace_bytes", "saber_k_rle_count", "saber_k_rle_encode", "saber_k_rle_decode"):
        assert re.search(r"\b" + name + r"\s*\(", kern), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "rle.hip" in open(os.path.join(ROOT, "saber_amd", "csrc", "Makefile")).read()
    need = lib.saber_k_rle_workspace_bytes(227, 1024, 1024)
    assert 227 * 1024 * 8 + 227 * 4 <= need <= 227 * 1024 * 8 + 227 * 4 + 3 * 256
    assert lib.saber_k_rle_workspace_bytes(0, 8, 8) == 0 and lib.saber_k_rle_workspace_bytes(1, 1 << 16, 1 << 15) == 0
    # argument errors are found before anything touches a device
    assert lib.saber_k_rle_count(None, 1, 8, 8, None, None, 0, None) == -1
    assert lib.saber_k_last_error().decode().startswith("rle_count:")
    assert lib.saber_k_rle_encode(None, 1, 8, 8, None, None, 0, None, 0, None) == -1
    assert lib.saber_k_last_error().decode().startswith("rle_encode:")
    assert lib.saber_k_rle_decode(None, None, 0, 8, 8, None, None) == -1
    assert lib.saber_k_last_error().decode().startswith("rle_decode:")
    assert "output_mode" not in [f[0] for f in _lib.AmgParams._fields_]


def test_engine_methods_fail_loudly_without_device():
    if torch.cuda.is_available():
        pytest.skip("has a GPU")
    from saber_amd.engine import Engine
    eng = Engine.__new__(Engine)                                     # no handle can be made without a device
    eng.h = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.rle_encode(torch.zeros((1, 4, 1), dtype=torch.int32), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.rle_decode(torch.zeros((1,), dtype=torch.int32), torch.zeros((2,), dtype=torch.int64), 4, 8)


class StubEngine:
    """returns two fixed masks; encodes with the restatement; records what it is asked for"""
    device = torch.device("cpu")

    def __init__(self, masks):
        from saber_amd import _lib
        self.masks = masks
        self.calls, self.encodes = [], 0
        self.meta = []
        for i, m in enumerate(masks):
            rec = _lib.MaskMeta(area=int(m.sum()), predicted_iou=0.9 - 0.1 * i, stability_score=0.95)
            self.meta.append(rec)

    def amg_generate(self, img, params, **kw):
        self.calls.append(kw)
        return torch.from_numpy(rle_ref.pack_bits(self.masks).view(np.int32)), list(self.meta)

    def rle_encode(self, bits, W):
        self.encodes += 1
        counts, offsets = rle_ref.encode_stack(rle_ref.unpack_bits(bits.numpy().view(np.uint32), W))
        return torch.from_numpy(counts.view(np.int32)), torch.from_numpy(offsets)


def test_output_mode_of_the_generator(monkeypatch):
    from saber_amd import engine as engine_mod
    from saber_amd.adapters.sam2 import automask, rle
    from saber_amd.segmenters.utils import DEVICE_ROW_KEY
    H, W = 8, 40
    masks = np.zeros((2, H, W), bool)
    masks[0, 2:5, 30:36] = True
    masks[1, 0, 0] = True
    img = np.zeros((H, W), np.float32)
    for bad in ("rle", "", None, "BINARY_MASK"):
        with pytest.raises(ValueError, match="output_mode"):
            automask.EngineMaskGenerator(StubEngine(masks), automask.get_default(), output_mode=bad)
    unpacked = []
    monkeypatch.setattr(engine_mod, "unpack_bits", lambda bits, w: unpacked.append(w) or rle_ref.unpack_bits(bits.numpy().view(np.uint32), w))
    # the default: bool arrays, no encode
    eng = StubEngine(masks)
    gen = automask.EngineMaskGenerator(eng, automask.get_default())
    assert gen.output_mode == "binary_mask"
    plain = gen.generate(img)
    assert unpacked == [W] and eng.encodes == 0 and eng.calls == [{"max_masks": 2048}]
    assert all(np.array_equal(d["segmentation"], m) for d, m in zip(plain, masks))
    # the RLE mode: dicts, no unpack, the mode never reaches the engine, every other key as before
    eng = StubEngine(masks)
    out = automask.EngineMaskGenerator(eng, automask.get_default(), output_mode="uncompressed_rle").generate(img)
    assert unpacked == [W] and eng.encodes == 1 and eng.calls == [{"max_masks": 2048}]
    assert len(out) == 2
    for d, p, m in zip(out, plain, masks):
        assert list(d) == list(p)
        assert d["segmentation"] == {"size": [H, W], "counts": rle_ref.encode(m)}
        assert np.array_equal(rle.rle_to_mask(d["segmentation"]), m) and rle.area_from_rle(d["segmentation"]) == d["area"]
        assert d[DEVICE_ROW_KEY][1] == p[DEVICE_ROW_KEY][1] and d[DEVICE_ROW_KEY][0].W == W
        assert {k: v for k, v in d.items() if k not in ("segmentation", DEVICE_ROW_KEY)} == {k: v for k, v in p.items() if k not in ("segmentation", DEVICE_ROW_KEY)}
    # no masks: nothing is encoded
    eng = StubEngine(masks[:0])
    assert automask.EngineMaskGenerator(eng, automask.get_default(), output_mode="uncompressed_rle").generate(img) == [] and eng.encodes == 0
    # build_amg
    eng = StubEngine(masks)
    monkeypatch.setattr(automask, "get_engine", lambda *a, **k: eng)
    cfg = dict(automask.get_default(), sam2_cfg="tiny")
    assert automask.build_amg(cfg, 50).base_generator.output_mode == "binary_mask"
    g = automask.build_amg(cfg, 0, output_mode="uncompressed_rle", min_mask_region_area=7)
    assert g.base_generator.output_mode == "uncompressed_rle"
    got = g.generate(img)
    assert [d["segmentation"]["counts"] for d in got] == [rle_ref.encode(m) for m in masks]
    assert eng.calls == [{"max_masks": 2048, "min_mask_region_area": 7}]
    with pytest.raises(ValueError, match="output_mode"):
        automask.build_amg(cfg, 50, output_mode="polygons")


def test_adapter_config_has_no_output_mode():
    from saber_amd.adapters.base import SAM2AdapterConfig
    assert "output_mode" not in SAM2AdapterConfig.model_fields
