"""GPU: the mask generator's small-region step (csrc/smallregions.hip; Engine.remove_small_regions, Engine.postprocess_small_regions,
Engine.amg_generate(min_mask_region_area=...)).  (a) saber_k_mask_small_regions on stacks whose answer is known by construction, (b) on
random stacks against the host restatement (tests/small_regions_ref.py), whole and chunked, (c) its error paths, (d) the engine-level
step on a bare handle, (e) one real output of the generator.  Every comparison is exact equality: the step moves bits and integers."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.small_regions_cases import constructed_cases
from tests.small_regions_ref import (RANDOM_CASES, expected_records, pack_bits, random_case, small_regions_ref, synthetic_meta, tight_box,
                                     unpack_bits)

pytestmark = pytest.mark.gpu

CASES = constructed_cases()
FILL = -0x55555556              # what outputs hold before a call: 0xAAAAAAAA


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def clean_dev(lib, masks, A, ws_masks=None, garbage_padding=False):
    """saber_k_mask_small_regions on masks (n,H,W) bool -> (new masks bool, changed, area, boxes) as numpy; checks that the input rows are
    left as they are and that the padding bits of the output are zero.  ws_masks: masks the workspace holds (None: all)"""
    n, H, W = masks.shape
    words = pack_bits(masks)
    if garbage_padding and W % 32:
        words = words.copy()
        words[..., -1] |= np.uint32((0xFFFFFFFF << (W % 32)) & 0xFFFFFFFF)
    src = torch.from_numpy(words.view(np.int32)).cuda()
    out = torch.full_like(src, FILL)
    changed = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    area = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    boxes = torch.full((n, 4), FILL, dtype=torch.int32, device="cuda")
    per = lib.saber_k_mask_small_regions_bytes(H, W)
    assert per >= H * W * 8 + H * ((W + 31) // 32) * 4
    ws = torch.empty(per * (n if ws_masks is None else ws_masks), dtype=torch.uint8, device="cuda")
    st = lib.saber_k_mask_small_regions(ptr(src), n, H, W, A, ptr(out), ptr(changed), ptr(area), ptr(boxes), ptr(ws), ws.numel(), None)
    torch.cuda.synchronize()
    assert st == 0, lib.saber_k_last_error().decode()
    assert np.array_equal(src.cpu().numpy().view(np.uint32), words)                  # the input is read only
    got = out.cpu().numpy().view(np.uint32)
    new = unpack_bits(got, W)
    assert np.array_equal(got, pack_bits(new)), "padding bits of the output are not zero"
    return new, changed.cpu().numpy(), area.cpu().numpy(), boxes.cpu().numpy()


def check(got, exp_masks, exp_changed, what):
    new, changed, area, boxes = got
    assert np.array_equal(new, exp_masks), f"{what}: {int((new != exp_masks).sum())} pixels differ"
    assert np.array_equal(changed, exp_changed.astype(np.int32)), f"{what}: changed {changed} != {exp_changed}"
    assert np.array_equal(area, exp_masks.reshape(len(exp_masks), -1).sum(1)), f"{what}: area"
    assert np.array_equal(boxes, np.array([tight_box(m) for m in exp_masks])), f"{what}: boxes"


# ------------------------------------------------------------------------------------------------ (a) constructed stacks
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_constructed_stacks(gpu_lib, case):
    name, masks, A, exp, exp_changed = case
    ref = small_regions_ref(masks, A)
    assert np.array_equal(ref["masks"], exp) and np.array_equal(ref["changed"], exp_changed)       # the restatement agrees with the construction
    check(clean_dev(gpu_lib, masks, A), exp, exp_changed, name)
    check(clean_dev(gpu_lib, masks, A, garbage_padding=True), exp, exp_changed, name + " (set padding bits)")


# ------------------------------------------------------------------------------------------------ (b) random stacks, whole and chunked
@pytest.mark.parametrize("case", RANDOM_CASES, ids=[str(c) for c in RANDOM_CASES])
def test_random_stacks_against_restatement(gpu_lib, case):
    masks, ref = random_case(case)
    n, A = case[1], case[4]
    n_changed, dropped = int(ref["changed"].sum()), n - len(ref["keep"])
    print(f"{case}: the restatement changes {n_changed} masks, its NMS drops {dropped}, keep list {ref['keep']}")
    assert n_changed >= n // 2 and dropped >= 2 and ref["keep"] != sorted(ref["keep"])
    whole = clean_dev(gpu_lib, masks, A)
    check(whole, ref["masks"], ref["changed"], "whole")
    chunked = clean_dev(gpu_lib, masks, A, ws_masks=2)
    check(chunked, ref["masks"], ref["changed"], "chunks of 2")
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ (c) error paths
def test_errors_write_nothing(gpu_lib):
    lib = gpu_lib
    masks = CASES[0][1]
    n, H, W = masks.shape
    src = torch.from_numpy(pack_bits(masks).view(np.int32)).cuda()
    out = torch.full_like(src, FILL)
    res = torch.full((6 * n,), FILL, dtype=torch.int32, device="cuda")
    ch, ar, bx = res[:n], res[n:2 * n], res[2 * n:]
    per = lib.saber_k_mask_small_regions_bytes(H, W)
    ws = torch.empty(per, dtype=torch.uint8, device="cuda")
    good = (ptr(src), n, H, W, 9, ptr(out), ptr(ch), ptr(ar), ptr(bx), ptr(ws), per)
    bad = {"workspace": {10: per - 1}, "min_area": {4: 0}, "min_area ": {4: -3}, "null in": {0: None}, "null out": {5: None}, "null changed": {6: None},
           "null area": {7: None}, "null box": {8: None}, "null workspace": {9: None}, "n = 0": {1: 0}, "H = 0": {2: 0}, "W < 0": {3: -1},
           "2^31 pixels": {2: 1 << 16, 3: 1 << 15, 10: 1 << 62}}
    for what, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.saber_k_mask_small_regions(*args, None) == -1, what
        msg = lib.saber_k_last_error().decode()
        assert msg.startswith("mask_small_regions:"), (what, msg)
        if what == "workspace":
            assert str(per) in msg                                 # the message names the size needed
    torch.cuda.synchronize()
    assert (out == FILL).all() and (res == FILL).all()
    assert lib.saber_k_mask_small_regions(*good, None) == 0          # the documented size is enough
    torch.cuda.synchronize()
    assert np.array_equal(unpack_bits(out.cpu().numpy().view(np.uint32), W), CASES[0][3])


# ------------------------------------------------------------------------------------------------ (d) the step on a bare handle
@pytest.fixture(scope="module")
def bare():
    from saber_amd.engine import Engine
    eng = Engine.bare(0)
    yield eng
    eng.close()


def to_ctypes(rec):
    from saber_amd import _lib
    assert rec.dtype.itemsize == C.sizeof(_lib.MaskMeta)
    arr = (_lib.MaskMeta * len(rec)).from_buffer_copy(np.ascontiguousarray(rec).tobytes())
    return [arr[i] for i in range(len(rec))]


def to_numpy(meta, dtype):
    return np.frombuffer(b"".join(bytes(m) for m in meta), dtype=dtype) if len(meta) else np.zeros(0, dtype)


@pytest.mark.parametrize("case", RANDOM_CASES, ids=[str(c) for c in RANDOM_CASES])
def test_engine_step_on_a_bare_handle(bare, case):
    masks, ref = random_case(case)
    seed, n, H, W, A = case
    rec = synthetic_meta(n)
    src = torch.from_numpy(pack_bits(masks).view(np.int32)).cuda()
    before = src.clone()
    bits, meta = bare.postprocess_small_regions(src, to_ctypes(rec), H, W, A, 0.7)
    assert torch.equal(src, before)
    keep = ref["keep"]
    assert len(meta) == len(keep) == bits.shape[0]
    got = bits.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, pack_bits(ref["masks"][keep]))                        # count, row order, bits, zero padding
    out = to_numpy(meta, rec.dtype)
    exp = expected_records(rec, ref)
    assert out.tobytes() == exp.tobytes()
    for i, k in enumerate(keep):
        if not ref["changed"][k]:
            assert out[i].tobytes() == rec[k].tobytes()                              # untouched survivors: byte for byte
        else:
            assert out[i]["area"] == ref["area"][k] and out[i]["bbox_xywh"].tolist() == [ref["boxes"][k][0], ref["boxes"][k][1], ref["boxes"][k][2] - ref["boxes"][k][0],
                                                                                         ref["boxes"][k][3] - ref["boxes"][k][1]]
            for f in ("predicted_iou", "stability_score", "point_xy", "crop_box_xywh"):
                assert out[i][f].tobytes() == rec[k][f].tobytes()
    # T = 1.0 drops nothing: all masks, untouched first, then changed, each group in its order
    bits1, meta1 = bare.postprocess_small_regions(src, to_ctypes(rec), H, W, A, 1.0)
    order = [i for i in range(n) if not ref["changed"][i]] + [i for i in range(n) if ref["changed"][i]]
    assert len(meta1) == n and np.array_equal(bits1.cpu().numpy().view(np.uint32), pack_bits(ref["masks"][order]))
    assert to_numpy(meta1, rec.dtype).tobytes() == expected_records(rec, dict(ref, keep=order)).tobytes()
    # the clean-up alone through the wrapper
    new, changed, area, boxes = bare.remove_small_regions(src, W, A)
    check((unpack_bits(new.cpu().numpy().view(np.uint32), W), changed.cpu().numpy(), area.cpu().numpy(), boxes.cpu().numpy()), ref["masks"],
          ref["changed"], "Engine.remove_small_regions")


def test_engine_step_arguments(bare):
    masks, ref = random_case(RANDOM_CASES[0])
    seed, n, H, W, A = RANDOM_CASES[0]
    src = torch.from_numpy(pack_bits(masks).view(np.int32)).cuda()
    meta = to_ctypes(synthetic_meta(n))
    bits, out = bare.postprocess_small_regions(src[:0], [], H, W, A, 0.7)            # no masks: nothing to do
    assert bits.shape[0] == 0 and out == []
    with pytest.raises(ValueError, match="min_area"):
        bare.postprocess_small_regions(src, meta, H, W, 0, 0.7)
    with pytest.raises(ValueError, match="records"):
        bare.postprocess_small_regions(src, meta[:-1], H, W, A, 0.7)
    with pytest.raises(ValueError, match="min_area"):
        bare.remove_small_regions(src, W, 0)
    from saber_amd import _lib
    cnt = C.c_int(7)
    rec = (_lib.MaskMeta * n)(*meta)
    st = bare.lib.saber_amg_postprocess_small_regions(bare.h, ptr(src), n, H, W, rec, A, 0.7, ptr(src), C.byref(cnt), None)
    assert st == -1 and "overlap" in bare.lib.saber_last_error(bare.h).decode() and cnt.value == 0


# ------------------------------------------------------------------------------------------------ (e) one real output of the generator
def test_real_generator_output(engine, image):
    from saber_amd.engine import make_amg_params
    from tests.small_regions_ref import nms_ref
    # the generator settings of tests/test_gpu_engine.py's golden comparison on this image: a 6 x 6 grid on one crop, box NMS off, so
    # that overlapping masks reach the step
    params = make_amg_params(dict(npoints=6, crop_n_layers=0, box_nms_thresh=1.0, pred_iou_thresh=0.5, stability_score_thresh=0.8))
    img = torch.from_numpy(image).cuda()
    H, W = image.shape
    bits, meta = engine.amg_generate(img, params, max_masks=512)
    n = len(meta)
    assert n > 0
    bits0, meta0 = engine.amg_generate(img, params, max_masks=512, min_mask_region_area=0)      # 0 = off: what the call without the keyword returns
    assert torch.equal(bits0, bits) and b"".join(bytes(m) for m in meta0) == b"".join(bytes(m) for m in meta)
    A = 25
    masks = unpack_bits(bits.cpu().numpy().view(np.uint32), W)
    ref = small_regions_ref(masks, A, 0.7)
    print(f"real generator output: {n} masks, {int(ref['changed'].sum())} changed by min_mask_region_area = {A}, {n - len(ref['keep'])} dropped by the "
          f"NMS at 0.7")
    dt = synthetic_meta(1).dtype
    rec = to_numpy(meta, dt)
    got_bits, got_meta = engine.postprocess_small_regions(bits, meta, H, W, A, 0.7)
    assert np.array_equal(got_bits.cpu().numpy().view(np.uint32), pack_bits(ref["masks"][ref["keep"]]))
    assert to_numpy(got_meta, dt).tobytes() == expected_records(rec, ref).tobytes()
    # the keyword applies the same step with T = max(box_nms_thresh, crop_nms_thresh) of the call's parameters: 1.0 here, nothing is dropped
    ref1 = dict(ref, keep=nms_ref(ref["boxes"], np.where(ref["changed"], 0.0, 1.0), 1.0))
    assert len(ref1["keep"]) == n
    on_bits, on_meta = engine.amg_generate(img, params, max_masks=512, min_mask_region_area=A)
    assert np.array_equal(on_bits.cpu().numpy().view(np.uint32), pack_bits(ref["masks"][ref1["keep"]]))
    assert to_numpy(on_meta, dt).tobytes() == expected_records(rec, ref1).tobytes()
