"""Host restatement of upstream's _apply_non_overlapping_constraints (sam2/modeling/sam2_base.py; SAM2Base(non_overlap_masks=True)
applies it to the video-resolution logits of every output) as saber_k_resize_planes_non_overlap and VideoPredictor(non_overlap_masks=True)
compute it: at every pixel the first object that attains the maximum keeps its logit, every other object reads min(logit, -10)."""
import numpy as np

SUPPRESS_MAX = np.float32(-10.0)


def non_overlap_ref(x: np.ndarray, suppress_max=SUPPRESS_MAX) -> np.ndarray:
    """x: (n, ...) float32 finite logits, objects along axis 0 (in obj_ids order).  Returns the constrained copy, same shape and dtype."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim >= 2
    if x.shape[0] == 1:
        return x.copy()
    winner = np.argmax(x, axis=0)                          # numpy, like torch.argmax, reports the first maximal index
    keep = np.arange(x.shape[0]).reshape((-1,) + (1,) * (x.ndim - 1)) == winner[None]
    return np.where(keep, x, np.minimum(x, np.float32(suppress_max))).astype(np.float32)


def overlap_pixels(x: np.ndarray) -> int:
    """pixels at which two or more objects are positive (what a label paint in object order resolves by id)"""
    return int(((np.asarray(x) > 0).sum(axis=0) >= 2).sum())
