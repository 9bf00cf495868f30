"""Host restatement of upstream's SAM2Transforms.postprocess_masks (sam2/utils/transforms.py, with get_connected_components of
sam2/utils/misc.py) as saber_k_clean_lowres and Engine.set_lowres_cleanup compute it.  Per plane x and threshold t: background is x <= t,
foreground is x > t (IEEE comparisons: -0.0 is background at t = 0, a NaN is in neither set); both are labelled 8-connected with scipy ON
THE ORIGINAL PLANE; with max_hole_area > 0 every pixel of a background component of AT MOST that many pixels becomes
float32(float64(t) + 10), with max_sprinkle_area > 0 every pixel of a foreground component of at most that many pixels
float32(float64(t) - 10); every other pixel keeps its bits.  No component is exempt at the border.

The second half builds the planes the host test (tests/test_lowres_cleanup_host.py, on this restatement) and the device test
(tests/test_gpu_lowres_cleanup.py, kernel against this restatement, bit for bit) share."""
import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3))


def fill_values(thr):
    """(value of a filled hole, value of a removed sprinkle) for the threshold thr"""
    t = np.float64(np.float32(thr))
    return np.float32(t + 10.0), np.float32(t - 10.0)


def clean_lowres_ref(x: np.ndarray, thr: float, max_hole_area: int, max_sprinkle_area: int) -> np.ndarray:
    """x: (..., H, W) float32.  Returns the cleaned copy."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim >= 2
    assert 0 <= max_hole_area <= 65535 and 0 <= max_sprinkle_area <= 65535
    t = np.float32(thr)
    hi, lo = fill_values(t)
    out = x.copy()
    planes_in, planes_out = x.reshape((-1,) + x.shape[-2:]), out.reshape((-1,) + x.shape[-2:])
    for src, dst in zip(planes_in, planes_out):
        with np.errstate(invalid="ignore"):
            sets = ((src <= t, max_hole_area, hi), (src > t, max_sprinkle_area, lo))      # both from the original values
        for member, max_area, value in sets:
            if max_area <= 0:
                continue
            label, n = ndimage.label(member, structure=EIGHT)
            small = np.bincount(label.ravel(), minlength=n + 1) <= max_area
            small[0] = False                               # label 0: the pixels outside this polarity
            dst[small[label]] = value
    return out


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ planes
SHAPES = ((1, 1), (3, 5), (17, 33), (64, 100), (255, 257), (256, 256))


def distinct(P, H, W, sign=1.0, base=1.0):
    """same sign everywhere, no two pixels equal (a pixel that lands in the wrong place shows)"""
    n = P * H * W
    return (sign * (base + np.arange(n, dtype=np.float64).reshape(P, H, W) / n)).astype(np.float32)


def checkerboard(H, W):
    yy, xx = np.mgrid[:H, :W]
    return np.where((yy + xx) % 2 == 0, 1.5, -1.5).astype(np.float32)[None]


def spiral(H, W):
    """a one-pixel-wide background spiral from the corner inwards with one-pixel foreground walls between its turns; (plane, its length)"""
    g = np.ones((H, W), np.float32)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y = x = d = 0
    g[0, 0] = -1.0
    n, turned = 1, 0

    def carved(yy, xx):
        return 0 <= yy < H and 0 <= xx < W and g[yy, xx] <= 0

    while turned < 2:
        dy, dx = dirs[d]
        ny, nx = y + dy, x + dx
        if 0 <= ny < H and 0 <= nx < W and not carved(ny, nx) and not carved(ny + dy, nx + dx):
            y, x = ny, nx
            g[y, x] = -1.0
            n, turned = n + 1, 0
        else:
            d, turned = (d + 1) % 4, turned + 1
    return g[None], n


def noise(seed, P, H, W, flip=0.03):
    """smooth random logits with 3 % of the pixels flipped in sign: many small and many large components of both polarities"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((P, H, W))
    x = np.stack([ndimage.uniform_filter(p, 7) for p in x]) * 12
    f = rng.random((P, H, W)) < flip
    x[f] = -x[f] - np.sign(x[f]) * 0.25
    return x.astype(np.float32)


def exact_sizes(H, W, a):
    """foreground plane with background rectangles of exactly a and a + 1 pixels (one pair inside, one pair on the border), and inside a
    large background block foreground pieces of a and a + 1 pixels; needs H >= 17, W >= 33 and a <= 12"""
    assert H >= 17 and W >= 33 and 1 <= a <= 12
    x = distinct(1, H, W)[0]
    x[2, 2:2 + a] = -1.0                       # a, inside
    x[4, 2:2 + a + 1] = -2.0                   # a + 1, inside
    x[0, 16:16 + a] = -3.0                     # a, on the top border
    x[H - 1, 16:16 + a + 1] = -4.0             # a + 1, on the bottom border
    x[7:10, W - 1] = -5.0                      # a pocket of 3 on the right border
    x[H - 1, 0] = -6.0                         # a corner pixel
    x[6:15, 0:14] = -7.0                       # a block of 126 background pixels with foreground pieces inside (109 stay background)
    x[8, 2:2 + a] = 3.0
    x[10, 2:2 + a + 1] = 4.0
    return x[None]


def hole_in_sprinkle():
    """a 5 x 5 foreground island (24 pixels) around a one-pixel hole, in a sea of background; with areas 30 / 30 the hole ends at t + 10
    inside an island at t - 10 (the two labellings do not see each other)"""
    x = distinct(1, 17, 33, sign=-1.0)[0]
    x[4:9, 6:11] = 2.0
    x[6, 8] = -0.5
    return x[None]


def special_values():
    """zeros of both signs, NaN pixels (of both signs) and the smallest denormals, for t = 0"""
    x = distinct(1, 17, 33)[0]
    x[1, 3] = 0.0
    x[1, 7] = -0.0
    x[3, 2:6] = 0.0
    x[3, 6:10] = -0.0                           # one run of 8 zeros of both signs
    x[5, 2:10] = -1.0
    x[5, 10] = np.nan                          # a NaN between two background runs of 8: two components
    x[5, 11:19] = -1.0
    x[7, 4] = -np.nan
    x[9, 5] = np.float32(1e-45)                # the smallest denormal is foreground
    x[9, 7] = np.float32(-1e-45)               # and its negative background
    x[11:14, 20:23] = np.nan                   # a ring of NaN around one foreground pixel: a sprinkle of 1 that touches nothing
    x[12, 21] = 5.0
    x[14, 2:8] = -2.0
    x[14, 4] = np.nan                          # NaN splits 6 into 2 + 3
    return x[None]


def threshold_half():
    """t = 0.5: 0.5 itself is background, the next float above it foreground"""
    x = distinct(1, 17, 33, base=2.0)[0]
    x[2, 2:6] = 0.5
    x[2, 6] = np.nextafter(np.float32(0.5), np.float32(1.0))      # foreground: ends the run
    x[2, 7:10] = 0.25
    x[6:12, 10:30] = 0.0
    x[8, 12:15] = 0.75                         # a sprinkle of 3 above 0.5
    x[10, 12:15] = 0.5                         # not one
    return x[None]


def adjacent_planes():
    """foreground in the last row of plane i directly above foreground in the first row of plane i + 1 (and a row's end against the next
    plane's first pixels): separate components"""
    x = distinct(3, 6, 37, sign=-1.0)
    for p in range(2):
        x[p, 5, 10:15] = 1.0
        x[p + 1, 0, 10:15] = 2.0
    x[0, 5, 32:37] = 3.0
    x[1, 0, 0:5] = 4.0
    return x


def kernel_cases():
    """(name, planes (P,H,W) float32, thr, max_hole_area, max_sprinkle_area)"""
    cases = []
    for (H, W) in SHAPES:
        n = H * W
        cb = checkerboard(H, W)
        nfg, nbg = (n + 1) // 2, n // 2
        for h, s in {(min(nbg, 65535), min(nfg, 65535)), (max(nbg - 1, 0), max(nfg - 1, 0)), (65535, 0), (0, 65535)}:
            if h or s:
                cases.append((f"checkerboard {H}x{W} h {h} s {s}", cb, 0.0, h, s))
        for sign in (1.0, -1.0):
            x = distinct(1, H, W, sign=sign)
            cases.append((f"all {'foreground' if sign > 0 else 'background'} {H}x{W} at 65535", x, 0.0, 65535, 65535))
            if n > 1:
                cases.append((f"all {'foreground' if sign > 0 else 'background'} {H}x{W} at n - 1", x, 0.0, min(n - 1, 65535), min(n - 1, 65535)))
        if H >= 17:
            g, length = spiral(H, W)
            walls = int((g > 0).sum())
            for h, s in ((length, 0), (length - 1, walls), (0, walls - 1), (min(length, 65535), min(walls, 65535))):
                cases.append((f"spiral {H}x{W} (length {length}, walls {walls}) h {h} s {s}", g, 0.0, h, s))
            ex = exact_sizes(H, W, 8)
            for h, s in ((8, 0), (0, 8), (8, 8), (9, 9), (3, 1)):
                cases.append((f"exact sizes {H}x{W} h {h} s {s}", ex, 0.0, h, s))
            nz = noise(H * 1000 + W, 2, H, W)
            for thr, h, s in ((0.0, 25, 25), (0.0, 8, 0), (0.0, 0, 8), (0.5, 300, 100), (-1.25, 1, 1)):
                cases.append((f"noise {H}x{W} t {thr} h {h} s {s}", nz, thr, h, s))
    cases.append(("3x5 pockets", np.array([[[-1, 1, 1, 1, -1], [1, 1, -1, 1, 1], [1, -1, 1, 1, -1]]], np.float32), 0.0, 2, 0))
    cases.append(("3x5 sprinkles", np.array([[[1, -1, -1, -1, 1], [-1, -1, 1, -1, -1], [-1, -1, -1, 1, -1]]], np.float32), 0.0, 0, 1))
    for h, s in ((30, 30), (30, 0), (0, 30), (1, 23), (1, 24)):
        cases.append((f"hole in a sprinkle h {h} s {s}", hole_in_sprinkle(), 0.0, h, s))
    for h, s in ((8, 8), (7, 0), (1, 1), (3, 0)):
        cases.append((f"zeros, signed zeros, NaN, denormals h {h} s {s}", special_values(), 0.0, h, s))
    for h, s in ((4, 3), (3, 2), (10, 10)):
        cases.append((f"t = 0.5 h {h} s {s}", threshold_half(), 0.5, h, s))
    for h, s in ((0, 5), (0, 4), (0, 10)):
        cases.append((f"adjacent planes h {h} s {s}", adjacent_planes(), 0.0, h, s))
    return cases
