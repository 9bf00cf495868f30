"""Hand-built mask stacks for the small-region step whose answer is known by construction: shared by the host test of the restatement
(tests/test_small_regions_host.py) and the device test of saber_k_mask_small_regions (tests/test_gpu_small_regions.py).
Every case is (name, masks (n,H,W) bool, A, expected masks (n,H,W) bool, expected changed (n,) bool); area and box follow from the
expected masks."""
import numpy as np

from tests.fill_holes_cases import spiral


def _body(H, W, margin=0):
    m = np.zeros((H, W), bool)
    m[margin:H - margin, margin:W - margin] = True
    return m


def _set(m, e, pixels, value, expect):
    for (y, x) in pixels:
        m[y, x] = value
        e[y, x] = expect


def _case(name, m, A, e, changed):
    m, e = np.asarray(m, bool), np.asarray(e, bool)
    if m.ndim == 2:
        m, e = m[None], e[None]
    return (name, m.copy(), A, e.copy(), np.atleast_1d(np.asarray(changed, bool)))


def constructed_cases():
    cases = []
    A = 9
    # holes of exactly A - 1 pixels are filled, of exactly A kept; on borders and in corners too (no border exception)
    m = _body(20, 37)
    e = m.copy()
    _set(m, e, [(3 + i, 4 + j) for i in range(2) for j in range(4)], False, True)                      # 2 x 4 = 8
    _set(m, e, [(3 + i, 12 + j) for i in range(3) for j in range(3)], False, False)                    # 3 x 3 = 9
    _set(m, e, [(9, 20 + j) for j in range(8)], False, True)
    _set(m, e, [(11, 20 + j) for j in range(9)], False, False)
    _set(m, e, [(0, 0), (0, 1), (1, 0)], False, True)                                                  # corners
    _set(m, e, [(19, 36), (18, 36), (19, 35), (18, 35)], False, True)
    _set(m, e, [(0, 36)], False, True)
    _set(m, e, [(19, 0), (19, 1)], False, True)
    _set(m, e, [(0, 15 + j) for j in range(5)], False, True)                                           # borders
    _set(m, e, [(19, 10 + j) for j in range(9)], False, False)
    _set(m, e, [(8 + i, 0) for i in range(8)], False, True)
    _set(m, e, [(5 + i, 36) for i in range(9)], False, False)
    cases.append(_case("holes: 8 filled, 9 kept, borders and corners", m, A, e, True))
    # the same shapes as islands on an empty plane next to a large body (so that "all below A" does not apply)
    m = np.zeros((24, 70), bool)
    m[2:22, 40:68] = True
    e = m.copy()
    _set(m, e, [(3 + i, 4 + j) for i in range(2) for j in range(4)], True, False)
    _set(m, e, [(3 + i, 12 + j) for i in range(3) for j in range(3)], True, True)
    _set(m, e, [(9, 20 + j) for j in range(8)], True, False)
    _set(m, e, [(11, 20 + j) for j in range(9)], True, True)
    _set(m, e, [(0, 0), (0, 1), (1, 0)], True, False)
    _set(m, e, [(23, 69), (22, 69)], True, False)
    _set(m, e, [(0, 69)], True, False)
    _set(m, e, [(23, 0), (23, 1)], True, False)
    _set(m, e, [(0, 25 + j) for j in range(9)], True, True)
    _set(m, e, [(23, 10 + j) for j in range(8)], True, False)
    _set(m, e, [(8 + i, 0) for i in range(9)], True, True)
    cases.append(_case("islands: 8 removed, 9 kept, borders and corners", m, A, e, True))
    # diagonal-only contacts join, both diagonals, both polarities
    for polarity in (False, True):                                 # False: the pieces are holes in a body, True: islands beside a body
        m = _body(26, 70) if not polarity else np.zeros((26, 70), bool)
        if polarity:
            m[2:24, 40:68] = True
        e = m.copy()
        small = not polarity                                       # what a region below A becomes: filled (True) or removed (False)
        _set(m, e, [(2, 3 + j) for j in range(5)] + [(3, 8 + j) for j in range(5)], polarity, polarity)             # "\": 10, stays
        _set(m, e, [(6, 8 + j) for j in range(5)] + [(7, 3 + j) for j in range(5)], polarity, polarity)             # "/": 10, stays
        _set(m, e, [(10, 3 + j) for j in range(4)] + [(11, 7 + j) for j in range(4)], polarity, small)              # 8
        _set(m, e, [(14, 7 + j) for j in range(4)] + [(15, 3 + j) for j in range(4)], polarity, small)              # 8
        _set(m, e, [(17 + i, 10 + i) for i in range(8)], polarity, small)                                          # pure "\" of 8
        _set(m, e, [(15 + i, 36 - i) for i in range(9)], polarity, polarity)                                       # pure "/" of 9
        cases.append(_case(f"diagonal contacts, {'islands' if polarity else 'holes'}", m, A, e, True))
    # runs across the word boundaries 31 | 32 and 63 | 64, both polarities
    for polarity in (False, True):
        m = _body(12, 130) if not polarity else np.zeros((12, 130), bool)
        if polarity:
            m[10:12, :] = True                                     # a band of 260 pixels
        e = m.copy()
        small = not polarity
        _set(m, e, [(1, c) for c in range(28, 36)], polarity, small)                                   # 8 across 31 | 32
        _set(m, e, [(3, c) for c in range(28, 37)], polarity, polarity)                                # 9
        _set(m, e, [(5, c) for c in range(60, 68)], polarity, small)                                   # 8 across 63 | 64
        _set(m, e, [(7, c) for c in range(60, 69)], polarity, polarity)                                # 9
        _set(m, e, [(1, c) for c in range(122, 130)], polarity, small)                                 # 8 up to the row's end
        _set(m, e, [(3, c) for c in range(121, 130)], polarity, polarity)
        _set(m, e, [(5, c) for c in range(0, 8)], polarity, small)                                     # 8 from the row's start
        cases.append(_case(f"runs across word boundaries, {'islands' if polarity else 'holes'}", m, A, e, True))
    # widths and heights, both polarities.  H = 5: rows 0, 2, 4 carry runs of the region's polarity, the full rows between them separate
    # the runs and join the rest of the plane into one large component.  H = 1: pieces along the line, alternately region and gap; every
    # gap has at least A pixels, so only the regions of 8 change.  W = 1: a column of single pixels, which the holes pass fills first
    for W in (1, 31, 32, 33, 37, 64, 70, 130):
        for H in (1, 5):
            for polarity in (False, True):                         # the regions are holes in a full plane / islands in an empty one
                m = np.full((2, H, W), not polarity)
                if W == 1:
                    m[:, 0::2, 0] = polarity
                    e = np.ones_like(m)                            # H 1: one pixel, filled or kept; H 5: the holes pass makes the column whole
                elif H == 1:
                    pieces = [8, 9, W - 17] if W < 64 else [8, 9, 9, 9, 8, W - 43]
                    e = m.copy()
                    x = 0
                    for i, k in enumerate(pieces):
                        if i % 2 == 0:
                            m[:, 0, x:x + k] = polarity
                            e[:, 0, x:x + k] = polarity if k >= A else not polarity
                        x += k
                else:
                    runs = [(0, 3), (5, 9), (16, 8), (W - 5, 5)] if W < 64 else [(0, 3), (5, 9), (16, 8), (28, 8), (40, 9), (W - 8, 8)]
                    if W == 130:
                        runs += [(58, 9), (70, 8)]
                    e = m.copy()
                    for y in range(0, H, 2):
                        for (x, k) in runs:
                            m[:, y, x:x + k] = polarity
                            e[:, y, x:x + k] = polarity if k >= A else not polarity
                cases.append(_case(f"rows of runs, {'islands' if polarity else 'holes'}, H {H} W {W}", m, A, e, [True, True]))
    # the ring: 8 pixels round a 1-pixel hole make an island of 9 once the hole is filled; a larger island is present
    m = np.zeros((12, 37), bool)
    m[1:4, 1:4] = True
    m[2, 2] = False
    m[6:10, 10:30] = True
    e = m.copy()
    e[2, 2] = True
    cases.append(_case("ring of 8 round a hole of 1, A 9: holes first", m, A, e, True))
    # a single island below A stays, pixel for pixel, and still counts as changed
    m = np.zeros((10, 33), bool)
    m[4, 30:33] = True
    cases.append(_case("a single island below A", m, A, m, True))
    # all islands below A: the unique largest stays; two equal largest: the first in raster order stays
    m = np.zeros((12, 40), bool)
    m[1, 1:4] = True
    m[5, 20:27] = True                                             # 7: the largest
    m[9, 5:10] = True
    e = np.zeros_like(m)
    e[5, 20:27] = True
    cases.append(_case("all islands below A, unique largest", m, A, e, True))
    m = np.zeros((12, 40), bool)
    m[1, 1:4] = True
    m[3, 30:37] = True                                             # 7, first pixel (3, 30)
    m[3:10, 2] = True                                              # 7, first pixel (3, 2): first in raster order
    e = np.zeros_like(m)
    e[3:10, 2] = True
    cases.append(_case("all islands below A, two equal largest", m, A, e, True))
    # an empty mask and a full mask: untouched
    cases.append(_case("empty mask", np.zeros((9, 37), bool), A, np.zeros((9, 37), bool), False))
    cases.append(_case("full mask", np.ones((9, 37), bool), A, np.ones((9, 37), bool), False))
    # a plane with H * W < A: whatever it holds, the holes pass fills it (an empty one too), and the full plane stays as the largest island
    for name, m in (("empty", np.zeros((2, 4), bool)), ("mixed", np.array([[1, 0, 0, 1], [0, 0, 1, 0]], bool))):
        cases.append(_case(f"plane of 8 pixels, {name}", m, A, np.ones((2, 4), bool), True))
    cases.append(_case("plane of 8 pixels, full", np.ones((2, 4), bool), A, np.ones((2, 4), bool), True))      # one island below A
    # a full-width band: the background above it (one row of 8 pixels) and below it (six rows) are separate components
    m = np.zeros((12, 8), bool)
    m[1:6, :] = True
    e = m.copy()
    e[0, :] = True
    cases.append(_case("full-width band, small background above it", m, A, e, True))
    # two stacked masks: 5 + 5 pixels in the facing rows would be one region of 10 if planes leaked; each is below A on its own
    m = np.ones((2, 6, 37), bool)
    m[0, 5, 10:15] = False
    m[1, 0, 10:15] = False
    m[0, 5, 32:37] = False                                         # a row's end and the next plane's first pixels
    m[1, 0, 0:5] = False
    cases.append(_case("planes do not leak, holes", m, A, np.ones((2, 6, 37), bool), [True, True]))
    m = np.zeros((2, 6, 37), bool)
    m[:, 2:4, 2:30] = True                                         # a body in each
    e = m.copy()
    m[0, 5, 10:15] = True
    m[1, 0, 10:15] = True
    m[0, 5, 32:37] = True
    m[1, 0, 0:5] = True
    cases.append(_case("planes do not leak, islands", m, A, e, [True, True]))
    # rows do not wrap: 5 pixels at a row's end and 5 at the next row's start are two regions of 5, not one of 10
    m = np.ones((9, 33), bool)
    m[2, 28:33] = False
    m[3, 0:5] = False
    cases.append(_case("rows do not wrap, holes", m, 10, np.ones((9, 33), bool), True))
    m = np.zeros((9, 33), bool)
    m[6:8, 3:30] = True
    e = m.copy()
    m[2, 28:33] = True
    m[3, 0:5] = True
    cases.append(_case("rows do not wrap, islands", m, 10, e, True))
    # the 64 x 64 one-pixel-wide spiral (n pixels) between one-pixel walls (one 8-connected component of w pixels), in both polarities
    g, n = spiral()
    s = g <= 0
    walls = ~s
    w = int(walls.sum())
    assert n > 1000 and w == 64 * 64 - n and 1000 < w < n - 1
    full = np.ones_like(s)
    # the spiral as the mask: at A = w the walls stay (a component of exactly A) and nothing is below A; from A = w + 1 on the walls are a
    # hole below A, the plane becomes full and stays as one island of 4096 pixels
    cases.append(_case("spiral mask, A the walls' size", s, w, s, False))
    cases.append(_case("spiral mask, A the walls' size + 1", s, w + 1, full, True))
    cases.append(_case("spiral mask, A its length - 1", s, n - 1, full, True))
    cases.append(_case("spiral mask, A its length", s, n, full, True))
    # the walls as the mask: the spiral is a hole of n pixels that stays up to A = n; the walls are a single island, which stays pixel for
    # pixel and counts as changed once A exceeds w; at A = n + 1 the spiral is filled
    cases.append(_case("spiral hole, A the walls' size", walls, w, walls, False))
    cases.append(_case("spiral hole, A the walls' size + 1", walls, w + 1, walls, True))
    cases.append(_case("spiral hole, A its length - 1", walls, n - 1, walls, True))
    cases.append(_case("spiral hole, A its length", walls, n, walls, True))
    cases.append(_case("spiral hole, A its length + 1", walls, n + 1, full, True))
    return cases
