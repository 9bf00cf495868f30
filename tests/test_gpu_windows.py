"""GPU: sliding-window masks on the device (csrc/windows.hip; Engine.place_window_masks, Engine.window_label_stack,
saber2D.segment_windows_device, segment_micrograph_core(device_windows=True)).
(a) every shift of a window against the frame's words at a ragged frame width, (b) windows narrower than, equal to and wider than a word,
(c) a window that is the frame, (d) two windows sharing output words, (e) 70 000 masks, (f) the engine entries' checks, (g) the route end to
end against the host route.  Every comparison is exact equality with the host restatement (tests/windows_ref.py) or the host route."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import windows_ref as ref

pytestmark = pytest.mark.gpu

FILL = -0x55555556              # what outputs hold before a call: 0xAAAAAAAA
GUARD = 64                      # guard words (place) / 16-byte groups of guard bytes (stack) on both sides


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def upload(src, table):
    s = torch.from_numpy(np.ascontiguousarray(src, dtype=np.uint32).view(np.int32)).cuda()
    t = torch.from_numpy(np.ascontiguousarray(table).view(np.uint8)).cuda()
    return s, t


def run_place(lib, src, table, H, W):
    """saber_k_place_window_masks into a filled stack with guard words on both sides, twice -> (n,H,W32) uint32"""
    n, W32 = len(table), (W + 31) // 32
    s, t = upload(src, table)
    outs = []
    for _ in range(2):
        buf = torch.full((GUARD + n * H * W32 + GUARD,), FILL, dtype=torch.int32, device="cuda")
        st = lib.saber_k_place_window_masks(ptr(s), ptr(t), n, H, W, ptr(buf[GUARD:]), None)
        assert st == 0, lib.saber_k_last_error().decode()
        torch.cuda.synchronize()
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n * H * W32:] == FILL).all(), "place wrote outside the stack"
        outs.append(buf[GUARD:GUARD + n * H * W32].cpu().numpy().view(np.uint32).reshape(n, H, W32))
    assert np.array_equal(s.cpu().numpy().view(np.uint32), src) and t.cpu().numpy().tobytes() == table.tobytes()       # inputs are read only
    assert outs[0].tobytes() == outs[1].tobytes(), "two calls differ"
    return outs[0]


def run_stack(lib, src, table, H, W, first, count, elem, shift=0):
    """saber_k_window_label_stack into a filled buffer with guard bytes on both sides, twice -> (count,H,W) unsigned array.
    shift: bytes the output base is moved off the 16-byte boundary (a multiple of elem)"""
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[elem]
    s, t = upload(src, table)
    nbytes, g = count * H * W * elem, 16 * GUARD + shift
    outs = []
    for _ in range(2):
        buf = torch.full((g + nbytes + 16 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        st = lib.saber_k_window_label_stack(ptr(s), ptr(t), first, count, H, W, elem, ptr(buf[g:]), None)
        assert st == 0, lib.saber_k_last_error().decode()
        torch.cuda.synchronize()
        assert (buf[:g] == 0xAA).all() and (buf[g + nbytes:] == 0xAA).all(), "stack wrote outside its planes"
        outs.append(buf[g:g + nbytes].cpu().numpy().view(dt).reshape(count, H, W))
    assert np.array_equal(s.cpu().numpy().view(np.uint32), src) and t.cpu().numpy().tobytes() == table.tobytes()
    assert outs[0].tobytes() == outs[1].tobytes(), "two calls differ"
    return outs[0]


def check_case(lib, masks, offsets, H, W, elems=(1, 2, 4), shift_elem=None):
    n = len(masks)
    exp_bits = ref.place(masks, offsets, H, W)
    full = ref.paste(masks, offsets, H, W)
    labels = np.arange(1, n + 1, dtype=np.uint32)[:, None, None]
    for padding in (False, True):
        what = f"frame {H} x {W}, source padding bits {'set' if padding else 'clean'}"
        src, table = ref.build_source(masks, offsets, padding)
        got = run_place(lib, src, table, H, W)
        bad = np.argwhere(got != exp_bits)
        assert bad.size == 0, f"{what}: place differs first at (mask, row, word) {bad[0].tolist()}, window {table[bad[0][0]]}"
        for elem in elems:
            if elem == 1 and n > 255:
                continue
            stack = run_stack(lib, src, table, H, W, 0, n, elem)
            bad = np.argwhere(stack != full * labels)
            assert bad.size == 0, f"{what}: stack of {elem}-byte elements differs first at {bad[0].tolist()}, window {table[bad[0][0]]}"
        if shift_elem is not None:                                                # the output base off the 16-byte boundary: element stores
            stack = run_stack(lib, src, table, H, W, 0, n, shift_elem, shift=shift_elem)
            assert np.array_equal(stack, full * labels), f"{what}: stack on a base moved by {shift_elem} bytes"
    return exp_bits, full


def random_masks(rng, shapes):
    return [rng.random(s) < 0.5 for s in shapes]


# ------------------------------------------------------------------------------------------------ (a) every shift, ragged frame width
def test_every_shift_at_a_ragged_width(gpu_lib):
    H, W, h, w = 40, 100, 17, 37
    offsets = [(y0, x0) for y0 in (0, 5, H - h) for x0 in (0, 1, 12, 31, 32, 33, 63)]
    assert max(x0 for _, x0 in offsets) + w == W
    rng = np.random.default_rng(1)
    masks = random_masks(rng, [(h, w)] * len(offsets))
    masks[3][:] = True                                                             # a full window: its rim is the test of every cut
    masks[4][:] = False
    _, full = check_case(gpu_lib, masks, offsets, H, W)
    # chunks: planes 3 .. 7 equal those of the whole stack, at every element size
    src, table = ref.build_source(masks, offsets, True)
    for elem in (1, 2, 4):
        whole = run_stack(gpu_lib, src, table, H, W, 0, len(masks), elem)
        assert np.array_equal(run_stack(gpu_lib, src, table, H, W, 3, 5, elem), whole[3:8])
        assert np.array_equal(whole[3:8], full[3:8] * np.arange(4, 9, dtype=np.uint32)[:, None, None])


# ------------------------------------------------------------------------------------------------ (b) widths around a word, h == 1
def test_widths_around_a_word(gpu_lib):
    H, W = 40, 100
    shapes, offsets = [], []
    for j, w in enumerate((1, 5, 31, 32, 33, 64)):
        for x0 in (0, 27):
            h = (1, 3, 40)[(j + (x0 > 0)) % 3]
            shapes.append((h, w))
            offsets.append((min(j * 7, H - h), x0))
    assert any(s[0] == 1 for s in shapes) and any(s == (40, 64) or s[0] == 40 for s in shapes)
    masks = random_masks(np.random.default_rng(2), shapes)
    masks[0][:] = True                                                             # 1 pixel wide: the word behind it belongs to the next row
    masks[1][:] = True
    check_case(gpu_lib, masks, offsets, H, W)


# ------------------------------------------------------------------------------------------------ (c) the window is the frame
def test_whole_frame_window(gpu_lib):
    masks = random_masks(np.random.default_rng(3), [(17, 37)])
    check_case(gpu_lib, masks, [(0, 0)], 17, 37)


# ------------------------------------------------------------------------------------------------ (d) two windows share output words
def test_windows_sharing_output_words(gpu_lib):
    H, W = 8, 64
    masks = [np.ones((3, 7), bool), np.ones((3, 7), bool)]
    masks[1][1, 3] = False
    offsets = [(1, 28), (2, 30)]                                                   # both straddle the boundary between words 0 and 1, rows 2 and 3 in common
    exp, full = check_case(gpu_lib, masks, offsets, H, W, shift_elem=4)
    assert (full[0] & full[1]).sum() > 0 and not np.array_equal(exp[0], exp[1])   # overlapping windows, independent planes
    check_case(gpu_lib, masks, offsets, H, W, elems=(1,), shift_elem=1)
    check_case(gpu_lib, masks, offsets, H, W, elems=(2,), shift_elem=2)


# ------------------------------------------------------------------------------------------------ (e) more masks than a grid dimension holds
def test_seventy_thousand_masks(gpu_lib):
    n, H, W, h, w = 70000, 16, 40, 8, 8
    rng = np.random.default_rng(4)
    stackm = rng.random((n, h, w)) < 0.5
    ys, xs = rng.integers(0, H - h + 1, n), rng.integers(0, W - w + 1, n)
    xs[:4] = (0, 24, 32, 31)
    masks, offsets = list(stackm), list(zip(ys.tolist(), xs.tolist()))
    exp_bits = ref.place(masks, offsets, H, W)
    full = ref.paste(masks, offsets, H, W)
    for padding in (False, True):
        src, table = ref.build_source(masks, offsets, padding)
        got = run_place(gpu_lib, src, table, H, W)
        bad = np.argwhere(got != exp_bits)
        assert bad.size == 0, f"place differs first at (mask, row, word) {bad[0].tolist()}"

        def expect(first, count):
            return full[first:first + count] * np.arange(first + 1, first + count + 1, dtype=np.uint32)[:, None, None]
        assert np.array_equal(run_stack(gpu_lib, src, table, H, W, 65530, 16, 4), expect(65530, 16))            # labels across 2^16
        assert np.array_equal(run_stack(gpu_lib, src, table, H, W, 65530, 5, 2), expect(65530, 5))             # up to 65535 in 2 bytes
        assert np.array_equal(run_stack(gpu_lib, src, table, H, W, 250, 5, 1), expect(250, 5))                 # up to 255 in 1 byte
        assert np.array_equal(run_stack(gpu_lib, src, table, H, W, 3, 5, 4), expect(3, 5))
        assert np.array_equal(run_stack(gpu_lib, src, table, H, W, n - 3, 3, 4), expect(n - 3, 3))
    s, t = upload(src, table)
    out = torch.full((64,), FILL, dtype=torch.int32, device="cuda")
    for first, count, elem in ((251, 5, 1), (65531, 5, 2), (0, 1, 3), (-1, 1, 4), (0, -1, 4)):
        assert gpu_lib.saber_k_window_label_stack(ptr(s), ptr(t), first, count, H, W, elem, ptr(out), None) == -1
        assert gpu_lib.saber_k_last_error().decode().startswith("window_label_stack:")
    assert gpu_lib.saber_k_place_window_masks(ptr(s), ptr(t), 1, 1 << 16, 1 << 15, ptr(out), None) == -1
    assert gpu_lib.saber_k_place_window_masks(ptr(s), ptr(t), 0, H, W, None, None) == 0
    assert gpu_lib.saber_k_window_label_stack(ptr(s), ptr(t), 7, 0, H, W, 4, None, None) == 0
    torch.cuda.synchronize()
    assert (out == FILL).all()


# ------------------------------------------------------------------------------------------------ (f) the engine entries
def test_engine_entries_check_every_record():
    from saber_amd import _lib
    from saber_amd.engine import Engine
    eng = Engine.bare(0)
    lib = eng.lib
    H, W = 40, 100
    rng = np.random.default_rng(5)
    shapes = [(17, 37), (1, 1), (40, 100), (3, 64)]
    offsets = [(5, 63), (39, 99), (0, 0), (37, 36)]
    masks = random_masks(rng, shapes)
    src, table = ref.build_source(masks, offsets, True)
    s = torch.from_numpy(src.view(np.int32)).cuda()
    good = [tuple(int(v) for v in r) for r in table]
    # the Python wrappers on valid input
    assert np.array_equal(eng.place_window_masks(s, good, H, W).cpu().numpy().view(np.uint32), ref.place(masks, offsets, H, W))
    st = eng.window_label_stack(s, good, H, W)
    assert st.dtype == torch.uint8 and np.array_equal(st.cpu().numpy(), ref.label_stack(masks, offsets, H, W))
    assert np.array_equal(eng.window_label_stack(s, good, H, W, first=1, count=2).cpu().numpy(), ref.label_stack(masks, offsets, H, W, 1, 2))
    many = good * 64                                             # 256 masks: 2-byte elements, chosen by the total, not by count
    st = eng.window_label_stack(s, many, H, W, first=254, count=2)
    assert st.dtype == torch.int16 and np.array_equal(st.cpu().numpy().view(np.uint16), ref.label_stack(masks * 64, offsets * 64, H, W, 254, 2))
    out = torch.full((2, H, W), 7, dtype=torch.int16, device="cuda")
    assert eng.window_label_stack(s, many, H, W, first=254, count=2, out=out) is out and torch.equal(out, st)
    with pytest.raises(ValueError):
        eng.window_label_stack(s, many, H, W, first=254, count=2, out=out.to(torch.int32))
    with pytest.raises(ValueError):
        eng.place_window_masks(s.cpu(), good, H, W)
    with pytest.raises(ValueError):
        eng.place_window_masks(s.to(torch.float32), good, H, W)

    # the C entries on invalid input: status, message, untouched output
    out = torch.full((len(good) * H * W,), FILL, dtype=torch.int32, device="cuda")      # room for four planes of 4-byte elements
    words = int(s.numel())
    y0, x0, h, w = 5, 63, 17, 37

    def place(records, src_words=words, H_=H, W_=W):
        return lib.saber_place_window_masks(eng.h, ptr(s), src_words, _lib.window_table(records), len(records), H_, W_, ptr(out), None)

    def stack(records, first, count, elem, src_words=words):
        return lib.saber_window_label_stack(eng.h, ptr(s), src_words, _lib.window_table(records), len(records), first, count, H, W, elem, ptr(out), None)
    bad_records = {"top": (0, -1, x0, h, w), "bottom": (0, H - h + 1, x0, h, w), "left": (0, y0, -1, h, w), "right": (0, y0, W - w + 1, h, w),
                   "src_word below": (-1, y0, x0, h, w), "src_word beyond": (words - h * 2 + 1, y0, x0, h, w), "h": (0, y0, x0, 0, w),
                   "w": (0, y0, x0, h, 0)}
    for name, rec in bad_records.items():
        for call in (lambda r: place(r), lambda r: stack(r, 0, len(r), 4)):
            assert call(good[:2] + [rec] + good[2:]) == _lib.SABER_ERR_INVALID, name
            assert "record 2" in lib.saber_last_error(eng.h).decode(), (name, lib.saber_last_error(eng.h).decode())
    assert place(good, src_words=words - 1) == _lib.SABER_ERR_INVALID and "record 3" in lib.saber_last_error(eng.h).decode()
    assert stack(good, 0, 4, 3) == _lib.SABER_ERR_INVALID
    assert stack(good * 64, 252, 4, 1) == _lib.SABER_ERR_INVALID                  # label 256 in one byte
    assert stack(good * 64, 65532, 4, 2) == _lib.SABER_ERR_INVALID                # first + count beyond the table (and label 65536 in two bytes)
    assert stack(good, 2, 3, 4) == _lib.SABER_ERR_INVALID                         # first + count beyond the table
    assert stack(good, -1, 2, 4) == _lib.SABER_ERR_INVALID and stack(good, 0, -1, 4) == _lib.SABER_ERR_INVALID
    assert place(good, H_=1 << 16, W_=1 << 15) == _lib.SABER_ERR_INVALID
    torch.cuda.synchronize()
    assert (out == FILL).all(), "an invalid call wrote to its output"             # nothing valid has touched `out` so far
    assert place([]) == 0 and stack(good, 1, 0, 4) == 0 and stack([], 0, 0, 1) == 0
    assert place(_lib.window_table([])) == 0
    torch.cuda.synchronize()
    assert (out == FILL).all(), "a call without masks wrote to its output"
    assert eng.place_window_masks(s, _lib.window_table([]), H, W).shape == (0, H, 4)           # an empty table converted beforehand stays empty
    assert eng.window_label_stack(s, [], H, W).shape == (0, H, W)
    assert stack(good * 64, 251, 4, 1) == 0                                       # label 255 fits one byte; the only call here that writes
    torch.cuda.synchronize()
    got = out.view(torch.uint8)[:4 * H * W].cpu().numpy().reshape(4, H, W)
    assert np.array_equal(got, ref.label_stack(masks * 64, offsets * 64, H, W, 251, 4, total=255))
    assert (out.view(torch.uint8)[4 * H * W:] == 0xAA).all()
    with pytest.raises(ValueError, match="record 0"):
        eng.place_window_masks(s, [bad_records["right"]], H, W)
    eng.close()


# ------------------------------------------------------------------------------------------------ (g) the route, end to end
@pytest.fixture(scope="module")
def micro():
    import os
    os.environ["SABER_AMD_SEEDED_WEIGHTS"] = "1"
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.amg import cfgAMG
    from saber_amd.segmenters.micro import cryoMicroSegmenter
    amg = cfgAMG(npoints=8, crop_n_layers=0, pred_iou_thresh=0.2, stability_score_thresh=0.3, sam2_cfg="small")

    def make(window_size, overlap_ratio):
        return cryoMicroSegmenter(deviceID=0, cfg=SAM2AdapterConfig(cfg="tiny", amg_cfg=amg, min_mask_area=50), min_mask_area=50,
                                  window_size=window_size, overlap_ratio=overlap_ratio)
    return make


def _image(S=448):
    """the micrograph of tests/test_gpu_dropin.py (_volume(Z=1, S=448)[0])"""
    rng = np.random.default_rng(11)
    vol = rng.normal(32768, 3000, (1, S, S))
    zz, yy, xx = np.mgrid[:1, :S, :S]
    for _ in range(9):
        cy, cx, r = rng.integers(40, S - 40, 2).tolist() + [int(rng.integers(15, 60))]
        vol[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += rng.choice([-6000, 6000])
    return np.clip(vol, 0, 65535).astype(np.float32)[0]


@pytest.mark.parametrize("geometry", ["448x448 window 256 overlap 0.25", "448x400 window 200 overlap 0.3"])
def test_device_route_equals_host_route(micro, geometry):
    from saber_amd.adapters.sam2.rle import rle_to_mask
    from saber_amd.filters.masks import masks_to_array
    if geometry.startswith("448x448"):
        img, seg = _image(), micro(256, 0.25)
        assert all(x1 % 32 == 0 for _, x1, _, _ in seg.get_sliding_windows(img.shape))
    else:
        img, seg = np.ascontiguousarray(_image()[:, :400]), micro(200, 0.3)
        wins = seg.get_sliding_windows(img.shape)
        assert sorted({x1 for _, x1, _, _ in wins}) == [0, 140, 280] and sorted({x2 - x1 for _, x1, _, x2 in wins}) == [120, 200]
    host = seg.segment(img, display=False, use_sliding_window=True)
    assert seg.window_masks is None
    seg.device_windows = True
    dev = seg.segment(img, display=False, use_sliding_window=True)
    wm = seg.window_masks
    print(f"{geometry}: {len(host)} masks on the host route, {len(dev)} on the device route")
    assert len(dev) == len(host) == len(wm) > 0
    for j, (d, h) in enumerate(zip(dev, host)):
        assert list(d.keys()) == list(h.keys()), j
        for k in h:
            if k == "segmentation":
                assert d[k].dtype == bool and d[k].shape == img.shape and np.array_equal(d[k], h[k]), j
            else:
                assert d[k] == h[k], (j, k, d[k], h[k])
    stack = wm.to_array_host(chunk=5)
    exp = masks_to_array(host)
    assert stack.dtype == exp.dtype and np.array_equal(stack, exp)
    rles = wm.rle()
    assert len(rles) == len(host)
    for r, h in zip(rles, host):
        assert r["size"] == list(img.shape) and np.array_equal(rle_to_mask(r), h["segmentation"])


def test_segment_micrograph_core_device_windows(micro, tmp_path):
    from saber_amd.entry_points.inference_core import segment_micrograph_core
    from saber_amd.utils import zarr_v2, zarr_writer
    from saber_amd.utils.mrc import write_mrc
    img = _image()
    write_mrc(str(tmp_path / "mic_002.mrc"), img, voxel_size=2.0)
    labels = {}
    for route in (False, True):
        seg = micro(256, 0.25)
        zarr_writer._zarr_writer = None
        out = str(tmp_path / f"out_{int(route)}.zarr")
        segment_micrograph_core(str(tmp_path / "mic_002.mrc"), out, None, None, False, True, 0, {"segmenter": seg}, device_windows=route)
        zarr_writer.get_zarr_writer(out).finalize()
        zarr_writer._zarr_writer = None
        run = zarr_v2.open_group(out)["mic_002"]
        labels[route] = run["labels"]["0"][:]
        if route:
            assert len(seg.window_masks) == labels[route].shape[0] == len(seg.masks) and all("segmentation" not in m for m in seg.masks)
    assert labels[True].shape[0] > 0 and labels[True].dtype == labels[False].dtype and np.array_equal(labels[True], labels[False])
