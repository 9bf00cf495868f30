"""CPU: the sliding-window device route's host side (saber_amd/segmenters/windows.py, Engine.window_label_stack's dtype rule, the
saber_window_mask record) against a fake engine that computes with the numpy restatement (tests/windows_ref.py).  The host route of
saber2D.segment_image runs on the same fake generator, so both lists are compared exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import windows_ref as ref


def test_window_mask_record_is_24_bytes():
    from saber_amd import _lib
    assert C.sizeof(_lib.WindowMask) == 24 == ref.TABLE_DTYPE.itemsize
    t = _lib.window_table([(7, 1, 2, 3, 4), (2 ** 40, 5, 6, 7, 8)])
    assert len(t) == 2 and (t[1].src_word, t[1].y0, t[1].x0, t[1].h, t[1].w) == (2 ** 40, 5, 6, 7, 8)
    assert bytes(t) == np.array([(7, 1, 2, 3, 4), (2 ** 40, 5, 6, 7, 8)], dtype=ref.TABLE_DTYPE).tobytes()
    assert _lib.window_table(t) is t
    assert len(_lib.window_table([])) == 0 and len(_lib.window_table(_lib.window_table([]))) == 0


def test_stack_dtype_follows_the_total_number_of_masks():
    from saber_amd.engine import window_stack_dtype
    assert window_stack_dtype(0) == window_stack_dtype(255) == torch.uint8
    assert window_stack_dtype(256) == window_stack_dtype(65535) == torch.int16
    assert window_stack_dtype(65536) == torch.int32
    from saber_amd.filters.masks import masks_to_array
    for n, dt in ((255, np.uint8), (256, np.uint16)):          # the rule it mirrors
        assert masks_to_array([{"segmentation": np.ones((1, 1), bool)}] * n).dtype == dt
        assert torch.empty(0, dtype=window_stack_dtype(n)).numpy().dtype.itemsize == np.dtype(dt).itemsize


def test_restatement_equals_rasterize_masks_and_masks_to_array():
    from saber_amd.filters.masks import masks_to_array
    from saber_amd.segmenters.base import saber2D
    rng = np.random.default_rng(3)
    H, W = 37, 70
    masks, offsets = [], []
    for h, w in ((5, 9), (37, 70), (1, 33), (12, 32), (7, 1)):
        masks.append(rng.random((h, w)) < 0.5)
        offsets.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))))
    host = saber2D.rasterize_masks(None, np.zeros((H, W)), [{"segmentation": m, "offset": o} for m, o in zip(masks, offsets)])
    for padding in (False, True):
        src, table = ref.build_source(masks, offsets, padding)
        back = ref.window_masks_of(src, table)
        placed = ref.unpack_rows(ref.place(back, offsets, H, W), W)
        for i, m in enumerate(host):
            assert np.array_equal(placed[i], m["segmentation"])
    assert (ref.place(masks, offsets, H, W)[:, :, -1] >> np.uint32(W % 32)).max() == 0          # clean padding at x >= W
    stack = masks_to_array(host)
    assert np.array_equal(ref.label_stack(masks, offsets, H, W), stack) and stack.dtype == np.uint8
    assert np.array_equal(ref.label_stack(masks, offsets, H, W, first=1, count=3), stack[1:4])


# ------------------------------------------------------------------------------------------------ the route on a fake engine
STABILITY = [0.9, 0.8, 0.7, 0.95, 0.6, 0.6, 0.5, 0.5]


class FakeEngine:
    """Engine + EngineMaskGenerator for the route: the "image" is an integer plane whose bit k is mask k; a window's masks are its non-empty
    bits in bit order.  Everything is computed with windows_ref on CPU tensors."""
    device = torch.device("cpu")

    def __init__(self):
        self.engine = self
        self.downloads = 0
        from saber_amd.adapters.sam2.automask import EngineMaskGenerator
        self.records = EngineMaskGenerator.records

    def _masks(self, image):
        v = np.asarray(image).astype(np.int64)
        return [(k, ((v >> k) & 1).astype(bool)) for k in range(len(STABILITY)) if ((v >> k) & 1).any()]

    def generate_device(self, image):
        from saber_amd import _lib
        found = self._masks(image)
        h, w = np.asarray(image).shape
        bits = ref.pack_rows(np.stack([m for _, m in found]), padding=True) if found else np.zeros((0, h, (w + 31) // 32), np.uint32)
        meta = []
        for k, m in found:
            ys, xs = np.nonzero(m)
            meta.append(_lib.MaskMeta(int(m.sum()), (float(xs.min()), float(ys.min()), float(xs.max() - xs.min()), float(ys.max() - ys.min())),
                                      0.5 + k / 100, STABILITY[k], (float(xs[0]), float(ys[0])), (0.0, 0.0, float(w), float(h))))
        return torch.from_numpy(bits.view(np.int32)), meta

    def generate(self, image):                                   # the host route's generator: the same masks as bool arrays
        bits, meta = self.generate_device(image)
        h, w = np.asarray(image).shape
        seg = ref.unpack_rows(bits.numpy().view(np.uint32), w)
        return [{"segmentation": seg[i], **r} for i, r in enumerate(self.records(meta))]

    def pair_intersections(self, bits, H, W):
        m = ref.unpack_rows(bits.numpy().view(np.uint32), W).reshape(bits.shape[0], -1).astype(np.int64)
        return torch.from_numpy((m @ m.T).astype(np.int32))

    def _full(self, src, table, H, W):
        t = np.array([(r.src_word, r.y0, r.x0, r.h, r.w) for r in table], dtype=ref.TABLE_DTYPE)        # WindowMasks hands over a _lib.window_table
        masks = ref.window_masks_of(src.numpy().view(np.uint32), t)
        return masks, [(int(r["y0"]), int(r["x0"])) for r in t]

    def place_window_masks(self, src, table, H, W):
        masks, offsets = self._full(src, table, H, W)
        return torch.from_numpy(ref.place(masks, offsets, H, W).view(np.int32))

    def window_label_stack(self, src, table, H, W, first=0, count=None, out=None):
        from saber_amd.engine import window_stack_dtype
        masks, offsets = self._full(src, table, H, W)
        a = ref.label_stack(masks, offsets, H, W, first=first, count=count)
        t = torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32}[a.dtype.itemsize]))
        assert t.dtype == window_stack_dtype(len(table))
        if out is not None:
            out.copy_(t)
            return out
        return t

    def unpack_masks(self, bits, W):
        return ref.unpack_rows(bits.numpy().view(np.uint32), W)


class FakeAdapter:
    def __init__(self, gen):
        self.gen = gen

    def _generator(self):
        return self.gen

    def segment_image_2d(self, image, text_prompt=None, threshold=None):
        return self.gen.generate(image)


def scene():
    """96 x 80 frame, window 64 / overlap 0.25: windows (0,0) 64x64, (0,48) 64x32, (48,0) 48x64, (48,48) 48x32 - nothing but the first is square"""
    img = np.zeros((96, 80), dtype=np.int64)

    def rect(bit, y, x, h, w):
        img[y:y + h, x:x + w] |= 1 << bit
    rect(0, 4, 4, 20, 30)       # 600 px, window (0,0) only
    rect(1, 30, 2, 5, 6)        # 30 px: between the two area thresholds
    rect(2, 50, 50, 10, 20)     # 200 px, a duplicate pair with bit 3 (IoU 0.95); seen by all four windows, cut differently
    rect(3, 50, 50, 10, 19)     # 190 px, the more stable of the two
    rect(4, 70, 10, 5, 9)       # 45 px  \ equal areas: generator (bit) order must survive the sort
    rect(5, 80, 20, 9, 5)       # 45 px  /
    rect(6, 90, 70, 2, 5)       # 10 px: below both thresholds
    rect(7, 66, 40, 3, 15)      # 45 px again, a third tie, straddling x = 48
    return img.astype(np.float32)


def make_segmenter(gen_min_area, seg_min_area):
    from saber_amd.adapters.sam2.amg import FilteredSAM2MaskGenerator
    from saber_amd.segmenters.base import saber2D
    fake = FakeEngine()
    seg = saber2D.__new__(saber2D)
    seg.min_mask_area, seg.window_size, seg.overlap_ratio = seg_min_area, 64, 0.25
    seg.classifier, seg.remove_repeating_masks, seg.device_windows, seg.window_masks = None, True, False, None
    seg.adapter = FakeAdapter(FilteredSAM2MaskGenerator(base_generator=fake, min_area_filter=gen_min_area))
    return seg, fake


@pytest.fixture()
def no_device_prepare(monkeypatch):
    from saber_amd.utils import preprocessing
    monkeypatch.setattr(preprocessing, "prepare", lambda image, to_rgb=False, engine=None: image)


@pytest.mark.parametrize("gen_min,seg_min", [(20, 40), (40, 20)])
def test_route_equals_host_route(no_device_prepare, gen_min, seg_min):
    from saber_amd.filters.masks import masks_to_array
    img = scene()
    seg, fake = make_segmenter(gen_min, seg_min)
    assert seg.get_sliding_windows(img.shape) == [(0, 0, 64, 64), (0, 48, 64, 80), (48, 0, 96, 64), (48, 48, 96, 80)]
    host = seg.segment_image(img, display=False, use_sliding_window=True)
    seg.device_windows = True
    dev = seg.segment_image(img, display=False, use_sliding_window=True)
    wm = seg.window_masks
    assert len(dev) == len(host) == len(wm) > 0
    for d, h in zip(dev, host):
        assert list(d.keys()) == list(h.keys()) and "_device_row" not in d
        for k in h:
            if k == "segmentation":
                assert d[k].dtype == bool and d[k].shape == img.shape and np.array_equal(d[k], h[k])
            else:
                assert d[k] == h[k], k
    # both area filters apply, whichever is the larger: nothing of 30 px (bit 1) or 10 px (bit 6) survives
    assert min(d["area"] for d in dev) >= 40
    # window order, then ascending area; the three 45-px masks keep generator (bit) order inside the window that sees them whole
    offs = [d["offset"] for d in dev]
    assert offs == sorted(offs) and set(offs) <= {(0, 0), (0, 48), (48, 0), (48, 48)}
    for o in set(offs):
        areas = [d["area"] for d in dev if d["offset"] == o]
        assert areas == sorted(areas)
    w3 = [d for d in dev if d["offset"] == (48, 0)]
    ties = [d for d in w3 if d["area"] == 45]
    assert [t["bbox"][:2] for t in ties] == [[10.0, 70.0], [20.0, 80.0], [40.0, 66.0]]         # bits 4, 5, 7, global x, y
    # bbox global, point_coords and crop_box window-local
    for d in dev:
        y1, x1 = d["offset"]
        ys, xs = np.nonzero(d["segmentation"])
        assert d["bbox"] == [float(xs.min()), float(ys.min()), float(xs.max() - xs.min()), float(ys.max() - ys.min())]
        assert d["crop_box"][:2] == [0.0, 0.0] and d["crop_box"][2] <= 64 and d["crop_box"][3] <= 64
        px, py = d["point_coords"][0]
        assert d["segmentation"][int(py) + y1, int(px) + x1]
    # the duplicate pair: one of the two stays per window - the more stable one, 190 px where the window (48, 48) sees both whole
    w4 = [d for d in dev if d["offset"] == (48, 48)]
    assert [d["area"] for d in w4] == [190] and [d["area"] for d in dev if d["offset"] == (0, 48)] == [190]
    assert sum(1 for d in w3 if d["area"] == 140) == 1
    # the other forms
    assert wm.records == [{k: v for k, v in d.items() if k != "segmentation"} for d in dev]
    stack = wm.to_array_host(chunk=3)
    assert stack.dtype == np.uint8 and np.array_equal(stack, masks_to_array(host))
    assert np.array_equal(wm.to_array(2, 3).numpy(), stack[2:5])
    assert np.array_equal(ref.unpack_rows(wm.bits().numpy().view(np.uint32), 80), np.stack([h["segmentation"] for h in host]))
    assert wm.bits() is wm.bits()
    words = sum(h * ((w + 31) // 32) for _, _, _, h, w in wm.table)
    assert wm.src.numel() == words and [t[0] for t in wm.table] == list(np.cumsum([0] + [t[3] * ((t[4] + 31) // 32) for t in wm.table])[:-1])


def test_classifier_is_refused_and_empty_result(no_device_prepare):
    seg, fake = make_segmenter(20, 40)
    seg.classifier = object()
    with pytest.raises(ValueError, match="classifier"):
        seg.segment_windows_device(scene())
    seg.classifier = None
    for empty_img in (np.zeros((96, 80), np.float32), np.where(scene().astype(np.int64) & 64, 64, 0).astype(np.float32)):     # nothing / only the 10-px mask
        wm = seg.segment_windows_device(empty_img)
        assert len(wm) == 0 and wm.dicts() == [] and wm.rle() == [] and wm.records == []
        assert wm.bits().shape == (0, 96, 3) and wm.to_array().shape == (0, 96, 80) and wm.to_array().dtype == torch.uint8
        a = wm.to_array_host()
        assert a.shape == (0, 96, 80) and a.dtype == np.uint8
        assert wm.src.numel() == 0
    with pytest.raises(ValueError):
        seg.segment_windows_device(np.zeros((96, 80, 4), np.float32))
