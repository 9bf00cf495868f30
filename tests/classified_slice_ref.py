"""Host restatements shared by the classified-slice tests (tests/test_classified_slices_host.py, tests/test_gpu_classified_slices.py):
bit packing of a mask stack as the mask generator lays it out, the plane the host route paints from convert_predictions_to_masks, and
the same plane from scipy's components plus the paint table of saber_amd.segmenters.slice_driver.classified_paint_lut."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "saber_classifier_glue.npz")


def pack_bits(stack: np.ndarray) -> np.ndarray:
    """(n,H,W) bool -> (n,H,ceil(W/32)) uint32, bit b of word w = pixel 32w+b (bit 1 of word 1 is pixel 33)"""
    n, H, W = stack.shape
    W32 = (W + 31) // 32
    padded = np.zeros((n, H, W32 * 32), dtype=bool)
    padded[..., :W] = stack
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<u4")


def golden_predictions() -> np.ndarray:
    """Synthetic class probabilities for the 8 masks of the golden fixture (areas 1403, 1117, 34297, 31, 526, 1369, 0, 1; 0 and 5
    overlap, 2 contains 0, 1, 5 and 7).  Class 1 owns 0, 5 (an overlapping pair) and 3 (31 pixels: below a min_area of 32); class 2 owns
    1, 2 (an overlapping pair), 4 and 7; the empty mask 6 is background.  Distinct float32 confidences."""
    p = np.array([[0.10, 0.70, 0.20], [0.05, 0.15, 0.80], [0.20, 0.25, 0.55], [0.30, 0.60, 0.10],
                  [0.10, 0.30, 0.60], [0.15, 0.45, 0.40], [0.90, 0.06, 0.04], [0.25, 0.05, 0.70]], dtype=np.float32)
    assert [int(v) for v in p.argmax(1)] == [1, 2, 2, 1, 2, 1, 0, 2]
    return p


def host_plane(fm, stack: np.ndarray, predictions: np.ndarray, target_class: int, min_area: int):
    """what slice_by_slice paints for one slice: convert_predictions_to_masks' dict list, idx + 1 in list order.  -> (plane, n)"""
    masks = [{"segmentation": m.astype(bool), "area": int(m.sum())} for m in stack]
    out = fm.convert_predictions_to_masks(predictions, masks, target_class, min_area)
    plane = np.zeros(stack.shape[1:], dtype=np.uint16)
    for idx, m in enumerate(out):
        plane[m["segmentation"]] = idx + 1
    return plane, len(out)


def restated_plane(stack: np.ndarray, predictions: np.ndarray, target_class: int, min_area: int):
    """the classifier branch of segment_slice_to_plane on the host: selection by argmax, components of the union (what the consensus
    kernels label), the paint table, the look-up.  -> (plane, n)"""
    from scipy import ndimage
    from saber_amd.segmenters.slice_driver import classified_paint_lut
    keep = [j for j, p in enumerate(np.argmax(predictions, axis=1)) if p == target_class]
    if not keep:
        return np.zeros(stack.shape[1:], dtype=np.uint16), 0
    labels, ncomp = ndimage.label(stack[keep].astype(bool).any(axis=0))
    areas = np.bincount(labels.ravel(), minlength=ncomp + 1)[1:]
    lut = classified_paint_lut(areas, min_area)
    return lut[labels], int(np.count_nonzero(lut))
