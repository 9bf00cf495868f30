"""Host side of the object-batched memory attention of the video path (saber_amd/adapters/sam2/video.py: batch_objects): the bank
signature and the grouping of a frame's objects on hand-written states, the new C-ABI symbols, and the switches' keywords.  No GPU."""
import inspect
import os
import re

import pytest

from saber_amd.adapters.sam2.video import VideoPredictor, bank_signature, group_by_signature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("saber_k_flash256_batched", "saber_k_rope_batched", "saber_k_membank_assemble", "saber_k_gemm_ld_batched")


def _state(cond, non_cond):
    return {"cond": {t: {} for t in cond}, "non_cond": {t: {} for t in non_cond}}


def test_signature_follows_the_selection_rules_of_the_per_object_route():
    # seeded on frame 2, tracked forward to frame 5 with num_maskmem = 2, 7 frames: one conditioning memory (slot 1), the previous frame's
    # memory (slot 0); pointers: the conditioning frame (offset 3), then frames 4, 3 (offsets 1, 2)
    st = _state([2], [3, 4])
    assert bank_signature(st, 5, False, 2, 7) == ((1, 0), (3, 1, 2))
    # the frame right after the seed: no tracked frame yet
    assert bank_signature(_state([2], []), 3, False, 2, 7) == ((1,), (1,))
    # reverse: frames above t count; a conditioning frame BELOW t gives a memory but no pointer
    assert bank_signature(_state([4], [2]), 1, True, 2, 7) == ((1, 0), (3, 1))
    assert bank_signature(_state([1], []), 3, True, 2, 7) == ((1,), ())
    # num_maskmem = 3: two temporal slots, farthest first, missing frames skipped
    assert bank_signature(_state([0], [1, 2]), 3, False, 3, 7) == ((2, 1, 0), (3, 1, 2))
    assert bank_signature(_state([0], [2]), 3, False, 3, 7) == ((2, 0), (3, 1))
    # the pointer scan stops at the volume's edge and at min(num_frames, 16) - 1 frames
    assert bank_signature(_state([0], list(range(1, 30))), 29, False, 2, 40) == ((1, 0), (29,) + tuple(range(1, 16)))
    assert bank_signature(_state([0], [1]), 2, False, 2, 3) == ((1, 0), (2, 1))


def test_equal_signatures_make_one_group_in_object_order():
    sig = ((1, 0), (3, 1, 2))
    assert group_by_signature([5, 2, 9], [sig, sig, sig], 16) == [[5, 2, 9]]


def test_a_different_pointer_count_makes_a_second_group():
    a, b = ((1, 0), (3, 1, 2)), ((1, 0), (1, 2))
    assert group_by_signature([1, 2, 3, 4], [a, b, a, b], 16) == [[1, 3], [2, 4]]
    # the memories' slots count as well
    assert group_by_signature([1, 2], [((1,), (1,)), ((0,), (1,))], 16) == [[1], [2]]
    # end to end from states: object 3 was seeded two frames later than objects 1 and 2
    states = {1: _state([2], [3, 4]), 2: _state([2], [3, 4]), 3: _state([4], [])}
    sigs = [bank_signature(states[o], 5, False, 2, 7) for o in (1, 2, 3)]
    assert group_by_signature([1, 2, 3], sigs, 16) == [[1, 2], [3]]


def test_groups_are_chunked_by_object_batch():
    a, b = ((1,), (1,)), ((1, 0), (2, 1))
    assert group_by_signature(list(range(5)), [a] * 5, 2) == [[0, 1], [2, 3], [4]]
    assert group_by_signature([1, 2, 3, 4, 5], [a, b, a, a, b], 2) == [[1, 3], [4], [2, 5]]
    assert group_by_signature([], [], 4) == []
    with pytest.raises(ValueError):
        group_by_signature([1], [a], 0)


def test_new_symbols_in_library_header_and_table(lib):
    from saber_amd import _lib
    header = open(os.path.join(ROOT, "include", "saber_amd_kernels.h")).read()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][1][-1] is _lib.C.c_void_p           # the stream comes last


def test_switches_are_keywords_with_the_route_off_by_default(monkeypatch):
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    from saber_amd.segmenters.base import saber3D
    p = inspect.signature(VideoPredictor.__init__).parameters
    assert p["batch_objects"].default in (None, False) and p["object_batch"].default == 16
    q = inspect.signature(SAM2Adapter.segment_volume).parameters
    assert q["batch_objects"].kind is inspect.Parameter.KEYWORD_ONLY and q["batch_objects"].default in (None, False)
    assert "self.batch_objects = False" in inspect.getsource(saber3D.__init__)
    src = inspect.getsource(VideoPredictor.__init__)
    assert "SABER_AMD_VIDEO_BATCH" in src
