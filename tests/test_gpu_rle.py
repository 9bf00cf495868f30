"""GPU: run-length output of the mask generator (csrc/rle.hip; Engine.rle_encode, Engine.rle_decode, EngineMaskGenerator(output_mode=...)).
(a) constructed stacks at sizes of one, two and three ballot steps with tails and ragged words, clean and set padding bits, (b) a stack
of more than 65 536 runs, (c) discs at 1024 x 1024, (d) the decoder, also on over-long counts behind guard words, (e) error paths and
repeatability, (f) one real output of the generator.  Every comparison is exact equality with the host restatement (tests/rle_ref.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import rle_ref

pytestmark = pytest.mark.gpu

FILL = -0x55555556              # what outputs hold before a call: 0xAAAAAAAA


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run_encode(lib, words, W, guard=16):
    n, H, W32 = words.shape
    src = torch.from_numpy(words.view(np.int32)).cuda()
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    need = lib.saber_k_rle_workspace_bytes(n, H, W)
    assert need >= n * W * 8 + n * 4
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = lib.saber_k_rle_count(ptr(src), n, H, W, ptr(offsets), ptr(ws), need, None)
    assert st == 0, lib.saber_k_last_error().decode()
    off = offsets.cpu().numpy()
    total = int(off[-1])
    buf = torch.full((total + guard,), FILL, dtype=torch.int32, device="cuda")
    st = lib.saber_k_rle_encode(ptr(src), n, H, W, ptr(offsets), ptr(buf), total, ptr(ws), need, None)
    assert st == 0, lib.saber_k_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy().view(np.uint32), words)                 # the input is read only
    assert (buf[total:] == FILL).all(), "entries behind offsets[n] were written"
    return buf[:total].cpu().numpy().view(np.uint32), off


def check_encode(lib, masks, names=None):
    n, H, W = masks.shape
    exp_counts, exp_off = rle_ref.encode_stack(masks)
    for padding in (False, True):
        counts, off = run_encode(lib, rle_ref.pack_bits(masks, padding=padding), W)
        what = f"{H} x {W}, padding bits {'set' if padding else 'clean'}"
        assert np.array_equal(off, exp_off), f"{what}: offsets {off.tolist()} != {exp_off.tolist()}"
        for i in range(n):
            got, exp = counts[off[i]:off[i + 1]], exp_counts[exp_off[i]:exp_off[i + 1]]
            assert np.array_equal(got, exp), f"{what}: mask {i} ({names[i] if names else ''}): {got[:8].tolist()}.. != {exp[:8].tolist()}.."
    return exp_counts, exp_off


def run_decode(lib, counts, offsets, H, W, guard=64):
    """saber_k_rle_decode into a stack with guard words on both sides -> (n,H,W32) uint32 words"""
    n = len(offsets) - 1
    W32 = (W + 31) // 32
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32)).cuda()
    o = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).cuda()
    buf = torch.full((guard + n * H * W32 + guard,), FILL, dtype=torch.int32, device="cuda")
    st = lib.saber_k_rle_decode(ptr(c), ptr(o), n, H, W, ptr(buf[guard:]), None)
    assert st == 0, lib.saber_k_last_error().decode()
    torch.cuda.synchronize()
    assert (buf[:guard] == FILL).all() and (buf[guard + n * H * W32:] == FILL).all(), "decode wrote outside the stack"
    return buf[guard:guard + n * H * W32].cpu().numpy().view(np.uint32).reshape(n, H, W32)


# ------------------------------------------------------------------------------------------------ (a) constructed stacks, (d) their decoding
@pytest.mark.parametrize("size", rle_ref.SIZES, ids=[f"{h}x{w}" for h, w in rle_ref.SIZES])
def test_constructed_stacks(gpu_lib, size):
    H, W = size
    names, masks = rle_ref.constructed_stack(H, W)
    assert names[:3] == ["checkerboard 0", "empty", "checkerboard 1"]              # an empty mask between two dense ones
    exp_counts, exp_off = check_encode(gpu_lib, masks, names)
    words = run_decode(gpu_lib, exp_counts, exp_off, H, W)                          # the restatement's counts
    assert np.array_equal(words, rle_ref.pack_bits(masks)), "decode: bits or padding differ"


# ------------------------------------------------------------------------------------------------ (b) more than 65 536 runs
def test_many_runs(gpu_lib):
    n, H, W = 5, 300, 257
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[:H, :W]
    masks = np.stack([rng.random((H, W)) < 0.5, (yy + xx) % 2 == 0, np.zeros((H, W), bool), yy % 2 == 1, rng.random((H, W)) < 0.3])
    exp_counts, exp_off = check_encode(gpu_lib, masks)
    assert exp_off[-1] > 65536 and np.diff(exp_off).max() > 65536
    assert np.array_equal(run_decode(gpu_lib, exp_counts, exp_off, H, W), rle_ref.pack_bits(masks))


# ------------------------------------------------------------------------------------------------ (c) discs at the generator's size
def test_discs_1024(gpu_lib):
    masks = rle_ref.discs(8)
    words = rle_ref.pack_bits(masks)
    counts, off = run_encode(gpu_lib, words, 1024)
    exp_counts, exp_off = rle_ref.encode_stack(masks)
    assert np.array_equal(off, exp_off) and np.array_equal(counts, exp_counts)
    assert np.array_equal(run_decode(gpu_lib, counts, off, 1024, 1024), words)      # decode(encode(bits)) == bits
    # two encodes give the same bytes
    again, off2 = run_encode(gpu_lib, words, 1024)
    assert again.tobytes() == counts.tobytes() and off2.tobytes() == off.tobytes()


# ------------------------------------------------------------------------------------------------ (d) decoder: round trip, malformed counts
def test_decode_round_trip_and_malformed_counts(gpu_lib):
    H, W = 130, 95
    names, masks = rle_ref.constructed_stack(H, W)
    counts, off = run_encode(gpu_lib, rle_ref.pack_bits(masks, padding=True), W)
    assert np.array_equal(run_decode(gpu_lib, counts, off, H, W), rle_ref.pack_bits(masks))       # zero padding whatever the input's held
    # over-long, short and empty runs: clamped at H W, zero behind the last run, nothing outside the stack (run_decode checks the guards)
    HW = H * W
    lists = [[0, HW + 77], [5, 2 ** 32 - 1, 9], [HW - 1, 50], [0, 0, 3, 0, 0, 4, 1], [10, 20], [HW + 5, 3], [0xFFFFFFFF] * 7,
             [3, 4, 0, 4, H - 11, 2 * H], [0, 32 * H, 0, 32 * H, 5, 0]]
    c = np.concatenate([np.asarray(v, dtype=np.uint32) for v in lists])
    o = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    got = rle_ref.unpack_bits(run_decode(gpu_lib, c, o, H, W), W)
    for i, v in enumerate(lists):
        assert np.array_equal(got[i], rle_ref.decode(v, H, W)), f"counts {v}"
    for hw in ((1, 1), (1, 70), (70, 1)):
        g = run_decode(gpu_lib, np.asarray([0, 10 ** 6, 1, 0], np.uint32), np.asarray([0, 2, 4]), *hw)
        assert np.array_equal(rle_ref.unpack_bits(g, hw[1]), np.stack([np.ones(hw, bool), np.zeros(hw, bool)]))


# ------------------------------------------------------------------------------------------------ (e) error paths
def test_errors_write_nothing(gpu_lib):
    lib = gpu_lib
    H, W = 65, 33
    names, masks = rle_ref.constructed_stack(H, W)
    n = len(masks)
    words = rle_ref.pack_bits(masks)
    src = torch.from_numpy(words.view(np.int32)).cuda()
    need = lib.saber_k_rle_workspace_bytes(n, H, W)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    good = (ptr(src), n, H, W, ptr(offsets), ptr(ws), need)
    bad = {"workspace": {6: need - 1}, "null bits": {0: None}, "null offsets": {4: None}, "null workspace": {5: None}, "n = 0": {1: 0}, "n < 0": {1: -2},
           "H = 0": {2: 0}, "W < 0": {3: -1}, "2^31 pixels": {2: 1 << 16, 3: 1 << 15, 6: 1 << 62}}
    for what, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.saber_k_rle_count(*args, None) == -1, what
        msg = lib.saber_k_last_error().decode()
        assert msg.startswith("rle_count:"), (what, msg)
        if what == "workspace":
            assert str(need) in msg                                # the message names the size needed
    torch.cuda.synchronize()
    assert (offsets == -7).all() and (ws == 0x5A).all()
    assert lib.saber_k_rle_count(*good, None) == 0                   # the documented size is enough
    exp_counts, exp_off = rle_ref.encode_stack(masks)
    assert np.array_equal(offsets.cpu().numpy(), exp_off)
    total = int(exp_off[-1])
    counts = torch.full((total,), FILL, dtype=torch.int32, device="cuda")
    good = (ptr(src), n, H, W, ptr(offsets), ptr(counts), total, ptr(ws), need)
    bad = {"workspace": {8: need - 1}, "capacity": {6: total - 1}, "capacity 0": {6: 0}, "null bits": {0: None}, "null offsets": {4: None},
           "null counts": {5: None}, "null workspace": {7: None}, "n = 0": {1: 0}, "H < 0": {2: -1}, "W = 0": {3: 0},
           "2^31 pixels": {2: 1 << 16, 3: 1 << 15, 8: 1 << 62}}
    for what, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.saber_k_rle_encode(*args, None) == -1, what
        msg = lib.saber_k_last_error().decode()
        assert msg.startswith("rle_encode:"), (what, msg)
        if what == "workspace":
            assert str(need) in msg
        if what == "capacity":
            assert str(total) in msg
    torch.cuda.synchronize()
    assert (counts == FILL).all()
    assert lib.saber_k_rle_encode(*good, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), exp_counts)
    out = torch.full_like(src, FILL)
    good = (ptr(counts), ptr(offsets), n, H, W, ptr(out))
    bad = {"null counts": {0: None}, "null offsets": {1: None}, "null bits": {5: None}, "n = 0": {2: 0}, "H = 0": {3: 0}, "W < 0": {4: -3},
           "2^31 pixels": {3: 1 << 16, 4: 1 << 15}}
    for what, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.saber_k_rle_decode(*args, None) == -1, what
        assert lib.saber_k_last_error().decode().startswith("rle_decode:"), what
    torch.cuda.synchronize()
    assert (out == FILL).all()
    assert lib.saber_k_rle_decode(*good, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), words)


# ------------------------------------------------------------------------------------------------ the engine's methods and the host helpers
def test_engine_methods(engine):
    from saber_amd.adapters.sam2 import rle
    H, W = 130, 95
    names, masks = rle_ref.constructed_stack(H, W)
    bits = torch.from_numpy(rle_ref.pack_bits(masks, padding=True).view(np.int32)).cuda()
    counts, offsets = engine.rle_encode(bits, W)
    exp_counts, exp_off = rle_ref.encode_stack(masks)
    assert counts.is_cuda and offsets.is_cuda and offsets.dtype == torch.int64
    assert np.array_equal(offsets.cpu().numpy(), exp_off) and np.array_equal(counts.cpu().numpy().view(np.uint32), exp_counts)
    dicts = rle.rle_dicts(counts, offsets, H, W)
    assert dicts == [{"size": [H, W], "counts": rle_ref.encode(m)} for m in masks]
    back = engine.rle_decode(counts, offsets, H, W)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), rle_ref.pack_bits(masks))
    assert np.array_equal(rle.rles_to_device(dicts, engine).cpu().numpy().view(np.uint32), rle_ref.pack_bits(masks))
    c0, o0 = engine.rle_encode(bits[:0], W)                                          # no masks: nothing to do
    assert c0.numel() == 0 and o0.tolist() == [0]
    with pytest.raises(ValueError, match="rle_encode"):
        engine.rle_encode(bits, W + 32)
    with pytest.raises(ValueError, match="rle_encode"):
        engine.rle_encode(bits.cpu(), W)
    with pytest.raises(ValueError, match="rle_decode"):
        engine.rle_decode(counts.to(torch.float32), offsets, H, W)
    with pytest.raises(ValueError, match="rle_decode"):
        engine.rle_decode(counts, offsets.to(torch.int32), H, W)
    with pytest.raises(ValueError, match="rle_decode"):
        engine.rle_decode(counts, offsets, 0, W)


# ------------------------------------------------------------------------------------------------ (f) one real output of the generator
def test_real_generator_output(engine, image):
    from saber_amd.adapters.sam2.automask import EngineMaskGenerator
    from saber_amd.adapters.sam2.rle import area_from_rle, rle_to_mask
    from saber_amd.segmenters.utils import DEVICE_ROW_KEY
    import saber_amd.engine as engine_mod
    # the generator settings of tests/test_gpu_small_regions.py::test_real_generator_output
    amg = dict(npoints=6, crop_n_layers=0, box_nms_thresh=1.0, pred_iou_thresh=0.5, stability_score_thresh=0.8)
    H, W = image.shape
    plain = EngineMaskGenerator(engine, amg, max_masks=512).generate(image)
    assert len(plain) > 0
    calls = []
    unpack = engine_mod.unpack_bits
    engine_mod.unpack_bits = lambda *a, **k: calls.append(a) or unpack(*a, **k)
    try:
        out = EngineMaskGenerator(engine, amg, max_masks=512, output_mode="uncompressed_rle").generate(image)
    finally:
        engine_mod.unpack_bits = unpack
    assert calls == [], "the RLE mode made bool arrays"
    assert len(out) == len(plain)
    print(f"real generator output: {len(out)} masks, {sum(len(d['segmentation']['counts']) for d in out)} run lengths")
    for d, p in zip(out, plain):
        assert list(d) == list(p)
        seg = d["segmentation"]
        assert seg["size"] == [H, W] and sum(seg["counts"]) == H * W
        assert np.array_equal(rle_to_mask(seg), p["segmentation"])
        assert area_from_rle(seg) == d["area"] == p["area"]
        assert torch.equal(d[DEVICE_ROW_KEY][0].bits[d[DEVICE_ROW_KEY][1]], p[DEVICE_ROW_KEY][0].bits[p[DEVICE_ROW_KEY][1]])
        rest = [k for k in d if k not in ("segmentation", DEVICE_ROW_KEY)]
        assert {k: d[k] for k in rest} == {k: p[k] for k in rest}
