"""Host restatement of the mask generator's small-region step (upstream SAM2AutomaticMaskGenerator.postprocess_small_regions with
remove_small_regions in both modes) as saber_k_mask_small_regions and saber_amg_postprocess_small_regions compute it, with numpy and
scipy.ndimage.label.  Per mask, A = min_area:
  1. holes: 8-connected background components with fewer than A pixels become foreground (no border exception);
  2. islands, on the result of 1: 8-connected foreground components with fewer than A pixels are removed; if all are below A the
     largest stays (first in scipy's numbering on a tie);
  3. changed = a component below A was met in 1 or 2 (also when no pixel differs); score 1 if unchanged else 0; box = tight box of the
     new mask with inclusive maxima, [0, 0, 0, 0] when empty;
  4. greedy NMS as torchvision.ops.nms: stable descending scores, fp32 IoU with area = (x2 - x1) (y2 - y1), suppressed when IoU > T;
  5. survivors in NMS order."""
import numpy as np
from scipy import ndimage

S8 = np.ones((3, 3), dtype=bool)


def pack_bits(masks: np.ndarray) -> np.ndarray:
    """(n,H,W) bool -> (n,H,ceil(W/32)) uint32, bit b of word w = pixel 32w+b, padding bits zero"""
    n, H, W = masks.shape
    W32 = (W + 31) // 32
    pad = np.zeros((n, H, W32 * 32), dtype=np.uint8)
    pad[..., :W] = masks
    return np.ascontiguousarray(np.packbits(pad, axis=-1, bitorder="little")).view(np.uint32).reshape(n, H, W32)


def unpack_bits(words: np.ndarray, W: int) -> np.ndarray:
    n, H, W32 = words.shape
    b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(n, H, W32 * 4), axis=-1, bitorder="little")
    return b[..., :W].astype(bool)


def clean_mask(m: np.ndarray, A: int):
    """one (H,W) bool mask -> (new mask, changed_h, changed_i)"""
    lab, k = ndimage.label(~m, structure=S8)
    sizes = np.bincount(lab.ravel(), minlength=k + 1)[1:]
    small = np.flatnonzero(sizes < A) + 1
    changed_h = small.size > 0
    m1 = m | np.isin(lab, small)
    lab, k = ndimage.label(m1, structure=S8)
    sizes = np.bincount(lab.ravel(), minlength=k + 1)[1:]
    changed_i = bool((sizes < A).any())
    keep = np.flatnonzero(sizes >= A) + 1
    if keep.size == 0 and k > 0:
        keep = np.array([int(np.argmax(sizes)) + 1])          # the first of the largest
    return np.isin(lab, keep), changed_h, changed_i


def tight_box(m: np.ndarray):
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return [0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def nms_ref(boxes: np.ndarray, scores: np.ndarray, thr: float):
    f = np.float32
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    order = np.argsort(-np.asarray(scores, dtype=np.float32), kind="stable")
    removed = np.zeros(len(order), dtype=bool)
    keep = []
    for a in range(len(order)):
        if removed[a]:
            continue
        i = order[a]
        keep.append(int(i))
        for c in range(a + 1, len(order)):
            if removed[c]:
                continue
            j = order[c]
            ia = f(f(b[i, 2] - b[i, 0]) * f(b[i, 3] - b[i, 1]))
            ja = f(f(b[j, 2] - b[j, 0]) * f(b[j, 3] - b[j, 1]))
            w = max(f(0), f(min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0])))
            h = max(f(0), f(min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1])))
            inter = f(w * h)
            with np.errstate(invalid="ignore", divide="ignore"):
                iou = f(inter) / f(f(ia + ja) - inter)
            if iou > f(thr):
                removed[c] = True
    return keep


def small_regions_ref(masks: np.ndarray, A: int, T: float = 0.7):
    """masks (n,H,W) bool -> dict: masks (n,H,W) bool, changed (n,) bool, area (n,), boxes (n,4) int, keep (list, NMS order)"""
    n = masks.shape[0]
    out = np.zeros_like(masks)
    changed = np.zeros(n, dtype=bool)
    boxes = np.zeros((n, 4), dtype=np.int64)
    for i in range(n):
        out[i], h, isl = clean_mask(masks[i], A)
        changed[i] = h or isl
        boxes[i] = tight_box(out[i])
    keep = nms_ref(boxes, np.where(changed, 0.0, 1.0), T)
    return {"masks": out, "changed": changed, "area": out.reshape(n, -1).sum(1).astype(np.int64), "boxes": boxes, "keep": keep}


def random_stack(seed, n, H, W, p=0.03):
    rng = np.random.default_rng(seed); yy, xx = np.mgrid[:H, :W]; out = np.zeros((n, H, W), bool)
    for i in range(n):
        k = i % 4
        if k in (0, 2):
            cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
            ry, rx = rng.uniform(0.12, 0.3) * H, rng.uniform(0.12, 0.3) * W
            base = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
        out[i] = base if k == 0 else base ^ (rng.random((H, W)) < p)
    return out


# (seed, n, H, W, A): at least n // 2 masks change, at least 2 are dropped by the NMS and the keep list is not ascending
RANDOM_CASES = ((0, 8, 64, 96, 10), (1, 12, 37, 70, 10), (2, 8, 130, 130, 25), (3, 16, 64, 64, 10), (4, 5, 33, 200, 10), (5, 32, 96, 160, 25))

_cache = {}


def random_case(case):
    """(masks, restatement) of one RANDOM_CASES entry, computed once per process and never modified by the tests"""
    if case not in _cache:
        seed, n, H, W, A = case
        m = random_stack(seed, n, H, W)
        r = small_regions_ref(m, A)
        m.setflags(write=False)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[case] = (m, r)
    return _cache[case]


def synthetic_meta(n):
    """records with distinct values in every field (numpy structured array with the layout of saber_mask_meta)"""
    dt = np.dtype([("area", np.int32), ("bbox_xywh", np.float32, 4), ("predicted_iou", np.float32), ("stability_score", np.float32),
                   ("point_xy", np.float32, 2), ("crop_box_xywh", np.float32, 4)])
    rec = np.zeros(n, dtype=dt)
    rec["area"] = 100000 + np.arange(n)
    rec["bbox_xywh"] = 0.5 + np.arange(4 * n, dtype=np.float32).reshape(n, 4)
    rec["predicted_iou"] = 0.7 + np.arange(n, dtype=np.float32) / 1000
    rec["stability_score"] = 0.9 + np.arange(n, dtype=np.float32) / 2000
    rec["point_xy"] = 3.25 + np.arange(2 * n, dtype=np.float32).reshape(n, 2)
    rec["crop_box_xywh"] = 7.0 + np.arange(4 * n, dtype=np.float32).reshape(n, 4)
    return rec


def expected_records(rec, ref):
    """the records the step must return for the input records `rec` and the restatement `ref`"""
    out = rec[ref["keep"]].copy()
    for i, k in enumerate(ref["keep"]):
        if ref["changed"][k]:
            x0, y0, x1, y1 = (int(v) for v in ref["boxes"][k])
            out["area"][i] = ref["area"][k]
            out["bbox_xywh"][i] = [x0, y0, x1 - x0, y1 - y0]
    return out
