"""CPU: non-overlapping masks of the video path - the host restatement (tests/non_overlap_ref.py) against upstream's literal torch
formula, the new C-ABI entry in the library, the header and the ctypes table, its argument refusals (answered without a device), and the
switches of VideoPredictor, SAM2AdapterConfig, SAM2Adapter.segment_volume and the 3-D segmenters."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.non_overlap_ref import SUPPRESS_MAX, non_overlap_ref, overlap_pixels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "saber_k_resize_planes_non_overlap"


def upstream(pred_masks: torch.Tensor) -> torch.Tensor:
    """SAM2Base._apply_non_overlapping_constraints, statement by statement"""
    batch_size = pred_masks.size(0)
    if batch_size == 1:
        return pred_masks
    device = pred_masks.device
    max_obj_inds = torch.argmax(pred_masks, dim=0, keepdim=True)
    batch_obj_inds = torch.arange(batch_size, device=device)[:, None, None, None]
    keep = max_obj_inds == batch_obj_inds
    pred_masks = torch.where(keep, pred_masks, torch.clamp(pred_masks, max=-10.0))
    return pred_masks


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check(x):
    want = upstream(torch.from_numpy(x)).numpy()
    got = non_overlap_ref(x)
    assert got.dtype == np.float32 and got.shape == x.shape and np.array_equal(_bits(got), _bits(want))
    return got


@pytest.mark.parametrize("n", [1, 2, 3, 17])
def test_restatement_is_the_torch_formula_on_random_stacks(n):
    x = (np.random.default_rng(n).standard_normal((n, 1, 7, 9)) * 8).astype(np.float32)
    got = _check(x)
    if n == 1:
        assert np.array_equal(_bits(got), _bits(x))
    else:
        assert overlap_pixels(x) > 0 and overlap_pixels(got) == 0
        assert ((got > SUPPRESS_MAX).sum(axis=0) <= 1).all()          # at most one object above -10 at a pixel


def test_the_first_object_keeps_its_value_on_a_tie():
    x = (np.random.default_rng(5).standard_normal((4, 1, 7, 9)) * 8).astype(np.float32)
    x[2] = x[0]                                                        # a tie across non-adjacent objects, everywhere
    x[1] = np.minimum(x[1], x[0] - 1)
    x[3, 0, :3] = x[0, 0, :3]                                          # three-way ties on the first rows
    got = _check(x)
    first = x[0] >= x[3]
    assert first.any() and np.array_equal(got[0][first], x[0][first])
    assert np.array_equal(got[2], np.minimum(x[2], SUPPRESS_MAX))      # the later twin always loses
    seeds = np.full((3, 1, 7, 9), -10.0, np.float32)                   # seed masks: +-10 logits; overlaps tie at +10
    seeds[0, 0, 1:5, 1:5] = seeds[1, 0, 3:7, 3:8] = seeds[2, 0, 2:4, 2:4] = 10.0
    got = _check(seeds)
    assert overlap_pixels(seeds) == 4 + 4 - 1 and overlap_pixels(got) == 0          # 0 with 1, 0 with 2, one pixel in all three
    assert (got[0] == seeds[0]).all() and (got[1, 0, 3:5, 3:5] == -10).all() and (got[2] == -10).all()


def test_losers_above_at_and_below_the_bound():
    x = np.empty((5, 1, 7, 9), np.float32)
    x[0] = 3.0                                                         # the winner
    x[1] = np.linspace(-9.99, 0.0, 63, dtype=np.float32).reshape(7, 9)      # losers in (-10, 0]
    x[2] = -10.0                                                       # exactly the bound
    x[3] = np.linspace(-500.0, -10.5, 63, dtype=np.float32).reshape(7, 9)   # below it: unchanged
    x[4] = -1024.0                                                     # an absent object's plane
    got = _check(x)
    assert (got[0] == 3.0).all() and (got[1] == -10.0).all() and np.array_equal(_bits(got[2:]), _bits(x[2:]))
    # a plane of -1024 changes nobody else: the constraint over the other planes alone gives the same planes
    assert np.array_equal(_bits(got[:4]), _bits(non_overlap_ref(x[:4])))
    x[:4] -= np.float32(2000.0)                                        # ... also where it is the winner: all others lie below -10 there
    assert (np.argmax(x, axis=0) == 4).all()
    got = _check(x)
    assert np.array_equal(_bits(got), _bits(x))
    y = np.concatenate([x[4:], x[:4]])                                 # and when it comes first
    assert np.array_equal(_bits(_check(y)), _bits(y))


def test_new_symbol_in_library_header_and_table(lib):
    from saber_amd import _lib
    assert getattr(lib, NAME) is not None
    header = open(os.path.join(ROOT, "include", "saber_amd_kernels.h")).read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", header)
    assert m, "not declared in include/saber_amd_kernels.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params == ["const float* in", "int n_planes", "int H", "int W", "float* out", "int Ho", "int Wo", "float suppress_max", "void* stream"]
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == args


def test_refusals_are_answered_without_a_device(lib):
    """argument errors are answered on the host (no launch, no device needed), with a message; the pointers are never followed"""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fn = getattr(lib, NAME)
    for args, word in (((None, 2, 4, 4, p, 4, 4), b"null"), ((p, 2, 4, 4, None, 4, 4), b"null"), ((p, -1, 4, 4, p, 4, 4), b"n_planes"),
                       ((p, 2, 0, 4, p, 4, 4), b"empty"), ((p, 2, 4, 0, p, 4, 4), b"empty"), ((p, 2, 4, 4, p, 0, 4), b"empty"),
                       ((p, 2, 4, 4, p, 4, 0), b"empty"), ((p, 2, 4, -3, p, 4, 4), b"empty"), ((p, 2, (1 << 22) + 1, 4, p, 4, 4), b"2^22")):
        assert fn(*args, -10.0, None) != 0, args
        msg = lib.saber_k_last_error()
        assert msg.startswith(b"resize_planes_non_overlap:") and word in msg, (args, msg)


def test_switches_are_off_by_default(monkeypatch):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    from saber_amd.adapters.sam2.video import VideoPredictor
    from saber_amd.segmenters.base import saber3D
    p = inspect.signature(VideoPredictor.__init__).parameters
    assert "non_overlap_masks" in p and p["non_overlap_masks"].default is None
    src = inspect.getsource(VideoPredictor.__init__)
    assert "SABER_AMD_NON_OVERLAP_MASKS" in src and "self.non_overlap_masks" in src
    assert callable(VideoPredictor._video_logits)
    assert NAME in inspect.getsource(VideoPredictor._video_logits)
    for fn in (VideoPredictor._frame_output, VideoPredictor.propagate_in_video):
        assert "_video_logits" in inspect.getsource(fn), fn.__name__
    assert SAM2AdapterConfig().non_overlap_masks is None and SAM2AdapterConfig(non_overlap_masks=True).non_overlap_masks is True
    q = inspect.signature(SAM2Adapter.segment_volume).parameters["non_overlap_masks"]
    assert q.kind is inspect.Parameter.KEYWORD_ONLY and q.default is None
    assert "non_overlap_masks=self._config.non_overlap_masks" in inspect.getsource(SAM2Adapter._video)
    assert "self.non_overlap_masks = False" in inspect.getsource(saber3D.__init__)
    assert '"non_overlap_masks"' in inspect.getsource(saber3D.propagate)
