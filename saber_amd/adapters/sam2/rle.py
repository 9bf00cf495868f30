"""Host side of the mask generator's run-length output (upstream: sam2/utils/amg.py mask_to_rle_pytorch, rle_to_mask, area_from_rle,
coco_encode_rle).  An uncompressed RLE is {"size": [H, W], "counts": [...]}: the mask flattened in column-major order (pixel (y, x) at
x H + y), runs of zeros and ones in turn, a zeros run first (0 when pixel (0,0) is set), summing to H W.  The encoding and the decoding of
whole stacks run on the device (Engine.rle_encode / Engine.rle_decode, csrc/rle.hip); here are the download into dicts, the upload
from dicts and the small per-dict helpers upstream has."""
from typing import Any, Dict, List, Sequence

import numpy as np

OUTPUT_MODES = ("binary_mask", "uncompressed_rle", "coco_rle")


def rle_dicts(counts, offsets, H: int, W: int) -> List[Dict[str, Any]]:
    """What Engine.rle_encode returned -> one {"size", "counts"} dict per mask.  One download: `offsets` rides behind `counts` in one
    int64-aligned device buffer."""
    import torch
    n = int(offsets.numel()) - 1
    if n <= 0:
        return []
    total = int(counts.numel())
    pad = total & 1                                            # keeps the offsets 8-byte aligned behind the 4-byte counts
    both = torch.empty((total + pad + 2 * (n + 1),), dtype=torch.int32, device=counts.device)
    both[:total] = counts.view(torch.int32)
    both[total + pad:] = offsets.view(torch.int32)
    host = both.cpu().numpy()
    off = host[total + pad:].view(np.int64)
    c = host[:total].view(np.uint32)
    if off[0] != 0 or off[-1] != total or (np.diff(off) < 1).any():
        raise ValueError(f"rle_dicts: offsets {off[:4].tolist()}.. do not partition {total} counts into {n} non-empty lists")
    return [{"size": [int(H), int(W)], "counts": c[off[i]:off[i + 1]].tolist()} for i in range(n)]


def _checked(rle):
    H, W = (int(v) for v in rle["size"])
    counts = np.asarray(rle["counts"], dtype=np.int64).reshape(-1)
    if H < 1 or W < 1 or counts.size < 1 or (counts < 0).any() or int(counts.sum()) != H * W:
        raise ValueError(f"uncompressed RLE: {counts.size} counts summing to {int(counts.sum())} for size [{H}, {W}]")
    return H, W, counts


def rle_to_mask(rle: Dict[str, Any]) -> np.ndarray:
    """{"size", "counts"} -> (H,W) bool array."""
    H, W, counts = _checked(rle)
    values = np.zeros(counts.size, dtype=bool)
    values[1::2] = True
    return np.repeat(values, counts).reshape(W, H).T


def area_from_rle(rle: Dict[str, Any]) -> int:
    return int(sum(rle["counts"][1::2]))


def rles_to_device(rles: Sequence[Dict[str, Any]], engine):
    """A list of uncompressed RLE dicts of one size -> the bit-packed (n,H,W32) int32 device stack (Engine.rle_decode).  Sizes must agree and
    every dict's counts must sum to H W (ValueError otherwise); one upload."""
    import torch
    if len(rles) == 0:
        raise ValueError("rles_to_device: no masks")
    H, W = (int(v) for v in rles[0]["size"])
    if H * W >= 2 ** 31:
        raise ValueError(f"rles_to_device: masks of 2^31 pixels or more are not supported, got [{H}, {W}]")
    parts = []
    for i, r in enumerate(rles):
        if [int(v) for v in r["size"]] != [H, W]:
            raise ValueError(f"rles_to_device: mask {i} has size {list(r['size'])}, mask 0 has [{H}, {W}]")
        parts.append(_checked(r)[2])
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([p.size for p in parts])
    total = int(offsets[-1])
    pad = total & 1
    host = np.zeros(total + pad + 2 * offsets.size, dtype=np.int32)
    host[:total] = np.concatenate(parts).astype(np.uint32).view(np.int32)
    host[total + pad:] = offsets.view(np.int32)
    dev = torch.from_numpy(host).to(engine.device)
    return engine.rle_decode(dev[:total], dev[total + pad:].view(torch.int64), H, W)


def coco_encode_rle(rle: Dict[str, Any]) -> Dict[str, Any]:
    """Uncompressed RLE -> COCO's compressed RLE ({"size", "counts": str}) through pycocotools, as upstream does; without pycocotools an
    ImportError that says so (no encoder of the compressed string is kept here)."""
    try:
        from pycocotools import mask as mask_utils
    except ImportError as e:
        raise ImportError("output_mode 'coco_rle' / coco_encode_rle needs pycocotools, which is not installed; use 'uncompressed_rle' "
                          "or install pycocotools") from e
    H, W = (int(v) for v in rle["size"])
    out = mask_utils.frPyObjects({"size": [H, W], "counts": list(rle["counts"])}, H, W)
    out["counts"] = out["counts"].decode("utf-8")
    return out
