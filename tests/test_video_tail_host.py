"""No GPU: the object-batched tail of a tracked video frame is wired through every layer - the two batched convolution entries are in the
built library, in the public header and in the ctypes table (stream last, as everywhere), and VideoPredictor carries the batch_tail switch
with its environment default."""
import ctypes as C
import inspect
import os
import re

from saber_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "saber_k_conv3x3s2_t_batched": ["const float*", "int64_t", "int", "int", "int", "const float*", "const float*", "int", "float*", "int64_t", "int", "void*"],
    "saber_k_dwconv7_t_batched": ["const float*", "int64_t", "int", "int", "int", "const float*", "const float*", "float*", "int64_t", "int", "void*"],
}
CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64}


def _header_args(name):
    src = open(os.path.join(ROOT, "include", "saber_amd_kernels.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/saber_amd_kernels.h"
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_batched_convolutions_are_in_the_header_the_table_and_the_library(lib):
    for name, types in ENTRIES.items():
        args = _header_args(name)
        assert [re.sub(r"\s*\w+$", "", a).replace(" *", "*") for a in args] == types, (name, args)
        assert args[-1] == "void* stream"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and list(argtypes) == [CTYPE[t] for t in types], name
        fn = getattr(lib, name)                    # resolved from the built libsaber_amd.so
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)


def test_batched_convolutions_refuse_before_they_touch_the_device(lib):
    """argument errors are answered on the host (no launch, no device needed), with a message"""
    assert lib.saber_k_conv3x3s2_t_batched(None, 64, 8, 8, 1, None, None, 4, None, 64, 1, None) != 0
    assert b"null" in lib.saber_k_last_error()
    assert lib.saber_k_dwconv7_t_batched(None, 64, 4, 4, 4, None, None, None, 64, 0, None) != 0
    assert b"batch" in lib.saber_k_last_error()


def test_video_predictor_has_the_batch_tail_switch():
    from saber_amd.adapters.sam2.video import VideoPredictor
    sig = inspect.signature(VideoPredictor.__init__)
    assert "batch_tail" in sig.parameters and sig.parameters["batch_tail"].default is None
    src = inspect.getsource(VideoPredictor.__init__)
    assert "SABER_AMD_VIDEO_BATCH_TAIL" in src and "self.batch_tail" in src
    for name in ("_track_tail_batch", "_encode_memory_batch", "_track_from", "_encode_memory", "_sam_heads"):
        assert callable(getattr(VideoPredictor, name)), name
