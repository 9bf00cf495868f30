"""Host restatement of upstream's fill_holes_in_mask_scores (sam2/utils/misc.py) as saber_k_fill_holes and
VideoPredictor(fill_hole_area=...) compute it: per plane, the 8-connected components of the background (x <= 0, so both zeros are
background and NaN is not) are labelled with scipy, and every pixel of a component of at most max_area pixels becomes float32(0.1)."""
import numpy as np
from scipy import ndimage

FILL_VALUE = np.float32(0.1)


def fill_holes_ref(x: np.ndarray, max_area: int, fill_value=FILL_VALUE):
    """x: (..., H, W) float32.  Returns (filled copy, number of components filled, number of components kept)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim >= 2
    out = x.copy()
    planes_in, planes_out = x.reshape((-1,) + x.shape[-2:]), out.reshape((-1,) + x.shape[-2:])
    filled = kept = 0
    for src, dst in zip(planes_in, planes_out):
        with np.errstate(invalid="ignore"):
            label, n = ndimage.label(src <= 0, structure=np.ones((3, 3)))
        area = np.bincount(label.ravel(), minlength=n + 1)
        small = area <= max_area
        small[0] = False                                   # label 0 is the foreground
        dst[small[label]] = fill_value
        filled += int(small[1:].sum())
        kept += int(n - small[1:].sum())
    return out, filled, kept


def random_planes(seed: int, shape):
    """Smooth random logits with sprinkled negative pixels: many small and many large background components per plane."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    x = np.stack([ndimage.uniform_filter(p, 5) for p in x.reshape((-1,) + tuple(shape[-2:]))]).reshape(shape)
    x = x * 10 + 1
    holes = rng.random(shape) < 0.03
    x[holes] = -np.abs(x[holes]) - 0.5
    return x.astype(np.float32)
