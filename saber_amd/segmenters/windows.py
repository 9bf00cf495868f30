"""The sliding-window branch of saber2D.segment_image (reference: saber/segmenters/base.py:103-150, 159-232) with the masks kept on the
device as the generator's bit-packed window rows.

The host route unpacks and downloads every window's masks, pastes each survivor into a full-frame bool array (rasterize_masks) and, in
segment_micrograph_core, multiplies every array into the (N, H, W) stack of filters.masks.masks_to_array.  Here a window's survivors are
chosen from per-mask scalars and one pair-intersection matrix (slice_driver.select_and_order), their rows are gathered into one ragged
device buffer, and what the caller asks for is written from those rows (csrc/windows.hip): full-frame bit-packed rows
(Engine.place_window_masks) or chunks of the label stack (Engine.window_label_stack).

    segment_windows   the per-window loop -> WindowMasks (collect_windows: its part behind the generator)
    WindowMasks       the result: ragged rows + one record per mask; bits() / to_array() / to_array_host() / rle() / dicts()
"""
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from saber_amd.segmenters import slice_driver


class WindowMasks:
    """The masks of a sliding-window run, in output order.
    src: 1-D int32 device tensor, the survivors' window rows one after another; table: per mask (src_word, y0, x0, h, w) - h rows of
    ceil(w / 32) words from src[src_word], pixel (0, 0) at frame pixel (y0, x0); records: the output dicts without `segmentation` (bbox
    in frame coordinates, offset = (y0, x0), point_coords and crop_box window-local as upstream leaves them); H, W: the frame.
    An empty result answers every method with the empty counterpart and launches nothing."""

    def __init__(self, engine, src: torch.Tensor, table: Sequence[Tuple[int, int, int, int, int]], records: List[Dict[str, Any]], H: int, W: int):
        if len(table) != len(records):
            raise ValueError(f"WindowMasks: {len(table)} table rows for {len(records)} records")
        self.engine, self.src, self.table, self.records, self.H, self.W = engine, src, list(table), records, int(H), int(W)
        from saber_amd import _lib
        self.table_c = _lib.window_table(self.table)          # what the engine calls take: converted once, not per chunk
        self._bits = None

    def __len__(self) -> int:
        return len(self.records)

    def bits(self) -> torch.Tensor:
        """(n, H, ceil(W/32)) int32 device tensor: every mask in full-frame bit-packed rows.  Placed on first use, then kept."""
        if self._bits is None:
            if len(self) == 0:
                self._bits = torch.empty((0, self.H, (self.W + 31) // 32), dtype=torch.int32, device=self.src.device)
            else:
                self._bits = self.engine.place_window_masks(self.src, self.table_c, self.H, self.W)
        return self._bits

    def to_array(self, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """planes first .. first + count - 1 of the masks_to_array stack as a device tensor (uint8 / int16 / int32 by the total number of
        masks: Engine.window_label_stack)"""
        n = len(self)
        count = n - first if count is None else count
        if first < 0 or count < 0 or first + count > n:
            raise ValueError(f"WindowMasks.to_array: planes {first} .. {first + count} of {n} masks")
        if count == 0:
            from saber_amd.engine import window_stack_dtype
            return torch.empty((0, self.H, self.W), dtype=window_stack_dtype(n), device=self.src.device)
        return self.engine.window_label_stack(self.src, self.table_c, self.H, self.W, first=first, count=count)

    def to_array_host(self, chunk: int = 64) -> np.ndarray:
        """The whole stack as the numpy array filters.masks.masks_to_array returns for dicts(): (n, H, W) uint8 / uint16 / uint32, mask j
        holding j + 1.  Written and downloaded `chunk` planes at a time, so at most that many exist on the device and no per-mask bool
        array is made anywhere."""
        n = len(self)
        if chunk < 1:
            raise ValueError("WindowMasks.to_array_host: chunk must be at least 1")
        np_dtype = np.uint8 if n < 256 else (np.uint16 if n < 65536 else np.uint32)
        out = np.zeros((n, self.H, self.W), dtype=np_dtype)
        if n == 0:
            return out
        from saber_amd.engine import window_stack_dtype
        k0 = min(chunk, n)
        dev = torch.empty((k0, self.H, self.W), dtype=window_stack_dtype(n), device=self.src.device)
        pin = torch.empty((k0, self.H, self.W), dtype=dev.dtype, pin_memory=True) if dev.is_cuda else None
        for first in range(0, n, k0):
            k = min(k0, n - first)
            self.engine.window_label_stack(self.src, self.table_c, self.H, self.W, first=first, count=k, out=dev[:k])
            if pin is None:
                host = dev[:k]
            else:
                pin[:k].copy_(dev[:k], non_blocking=True)
                torch.cuda.current_stream(dev.device).synchronize()
                host = pin[:k]
            out[first:first + k] = host.numpy().view(np_dtype)
        return out

    def rle(self, output_mode: str = "uncompressed_rle") -> List[Dict[str, Any]]:
        """every mask's full-frame `segmentation` in the generator's RLE output modes ({"size", "counts"}; Engine.rle_encode over bits())"""
        from saber_amd.adapters.sam2 import rle
        if output_mode not in ("uncompressed_rle", "coco_rle"):
            raise ValueError(f"WindowMasks.rle: output_mode must be 'uncompressed_rle' or 'coco_rle', got {output_mode!r}")
        if len(self) == 0:
            return []
        counts, offsets = self.engine.rle_encode(self.bits(), self.W)
        out = rle.rle_dicts(counts, offsets, self.H, self.W)
        return [rle.coco_encode_rle(r) for r in out] if output_mode == "coco_rle" else out

    def dicts(self) -> List[Dict[str, Any]]:
        """The list the host route returns: every record with its full-frame bool `segmentation` first (unpacked on the device from bits(),
        Engine.unpack_masks); no device-row key."""
        if len(self) == 0:
            return []
        seg = self.engine.unpack_masks(self.bits(), self.W)
        return [{"segmentation": seg[i], **rec} for i, rec in enumerate(self.records)]


def _wrapper_filters(gen, records: List[Dict[str, Any]], h: int, w: int) -> List[Dict[str, Any]]:
    """FilteredSAM2MaskGenerator.generate's filters (saber/adapters/sam2/amg.py:161-183) on records instead of dicts: both read scalars only"""
    fu = gen.filter_utils
    if gen.max_rel_box_size is not None or gen.min_rel_box_size is not None:
        records = fu.filter_masks_by_relative_box_size(records, max_rel_box_size=gen.max_rel_box_size, min_rel_box_size=gen.min_rel_box_size,
                                                       image_height=h, image_width=w)
    if gen.min_area_filter is not None or gen.max_area_filter is not None:
        records = fu.filter_masks_by_area(records, min_area=gen.min_area_filter, max_area=gen.max_area_filter)
    return records


def collect_windows(gen, generated, H: int, W: int, min_mask_area: int, remove_repeating_masks: bool = True) -> WindowMasks:
    """Everything of the route that follows the generator.  generated: an iterable of ((y1, x1, y2, x2), bits, meta), a window and what
    EngineMaskGenerator.generate_device returned for it, in output order."""
    base = gen.base_generator
    engine = base.engine
    parts, table, records = [], [], []
    word = 0
    for (y1, x1, y2, x2), bits, meta in generated:
        h, w = y2 - y1, x2 - x1
        w32 = (w + 31) // 32
        recs = base.records(meta)
        for i, r in enumerate(recs):
            r["_row"] = i
        recs = [r for r in _wrapper_filters(gen, recs, h, w) if r["area"] >= min_mask_area]
        if not recs:
            continue
        rows = [r.pop("_row") for r in recs]
        sel = bits[torch.as_tensor(rows, dtype=torch.long, device=bits.device)].contiguous()
        inter = engine.pair_intersections(sel, h, w).cpu().numpy() if remove_repeating_masks else None
        order = slice_driver.select_and_order([meta[i] for i in rows], inter, min_mask_area, remove_repeating_masks)
        if not order:
            continue
        parts.append(sel[torch.as_tensor(order, dtype=torch.long, device=sel.device)].reshape(-1))
        for k in order:
            r = recs[k]
            x, y, bw, bh = r["bbox"]
            r["bbox"] = [x + x1, y + y1, bw, bh]
            r["offset"] = (y1, x1)
            records.append(r)
            table.append((word, y1, x1, h, w))
            word += h * w32
    src = torch.cat(parts) if parts else torch.empty((0,), dtype=torch.int32, device=engine.device)
    return WindowMasks(engine, src, table, records, H, W)


def segment_windows(image: np.ndarray, windows: Sequence[Tuple[int, int, int, int]], gen, min_mask_area: int,
                    remove_repeating_masks: bool = True) -> WindowMasks:
    """saber2D.segment_image(use_sliding_window=True) without a classifier, on the device.
    image: (H,W) or (H,W,3); windows: (y1, x1, y2, x2) in output order (saber2D.get_sliding_windows); gen: the adapter's
    FilteredSAM2MaskGenerator over an EngineMaskGenerator; min_mask_area: the segmenter's (the generator's own area filter applies too:
    the filters are conjunctive).  Per window, in the host route's order: prepare on the window alone, generate_device, the wrapper's
    filters, area >= min_mask_area, duplicate removal and the stable ascending-area sort (slice_driver.select_and_order on the masks that
    are left), then the survivors' rows are gathered behind those of the windows before.  One download per window - the intersection
    matrix of the masks that reach the duplicate removal - and none of any mask."""
    if image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3):
        raise ValueError(f"segment_windows: expected (H,W) or (H,W,3), got {image.shape}")
    from saber_amd.utils import preprocessing
    base = gen.base_generator

    def generated():
        for win in windows:
            window = image[win[0]:win[2], win[1]:win[3]]
            bits, meta = base.generate_device(preprocessing.prepare(window, to_rgb=window.ndim == 2, engine=base.engine))
            yield win, bits, meta
    return collect_windows(gen, generated(), image.shape[0], image.shape[1], min_mask_area, remove_repeating_masks)
