"""Hand-built planes for hole filling whose answer is known by construction (max_area = 8 unless a case says otherwise): shared by the
host test of the restatement (tests/test_fill_holes_host.py) and the device test of saber_k_fill_holes (tests/test_gpu_fill_holes.py).
Every case is (name, x (planes, H, W) float32, max_area, expected (planes, H, W) float32); compare int32 views."""
import numpy as np

FILL = np.float32(0.1)


def _plane(P, H, W):
    """positive everywhere, no two pixels equal (a pixel that lands in the wrong place shows)"""
    return (1.0 + np.arange(P * H * W, dtype=np.float32).reshape(P, H, W) / np.float32(P * H * W)).astype(np.float32)


def _carve(x, exp, pixels, filled, plane=0, value=-1.0):
    for (y, xx) in pixels:
        x[plane, y, xx] = value
        exp[plane, y, xx] = FILL if filled else value


def _rows(P, H, W, runs_per_row):
    """rows 0, 2, 4, ... carry background runs (start, length), the rows between them are positive: the components are the runs"""
    x = _plane(P, H, W)
    exp = x.copy()
    for p in range(P):
        for y in range(0, H, 2):
            for (s, n) in runs_per_row:
                if s + n <= W:
                    _carve(x, exp, [(y, c) for c in range(s, s + n)], n <= 8, plane=p, value=-1.0 - y)
    return x, exp


def spiral(H=64, W=64):
    """a one-pixel-wide background spiral from the corner inwards, one-pixel walls between its turns; returns (plane, its length)"""
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
    return g, n


def constructed_cases():
    cases = []
    # holes of exactly 8 pixels are filled, of exactly 9 kept; holes on the border and in the corners
    x = _plane(1, 20, 37)
    exp = x.copy()
    _carve(x, exp, [(3 + i, 4 + j) for i in range(2) for j in range(4)], True)                        # 2 x 4 = 8
    _carve(x, exp, [(3 + i, 12 + j) for i in range(3) for j in range(3)], False)                      # 3 x 3 = 9
    _carve(x, exp, [(9, 20 + j) for j in range(8)], True)                                             # a run of 8
    _carve(x, exp, [(11, 20 + j) for j in range(9)], False)                                           # a run of 9
    _carve(x, exp, [(0, 0), (0, 1), (1, 0)], True)                                                    # corners
    _carve(x, exp, [(19, 36), (18, 36), (19, 35), (18, 35)], True)
    _carve(x, exp, [(0, 36)], True)
    _carve(x, exp, [(19, 0), (19, 1)], True)
    _carve(x, exp, [(0, 15 + j) for j in range(5)], True)                                             # borders
    _carve(x, exp, [(19, 10 + j) for j in range(9)], False)
    _carve(x, exp, [(8 + i, 0) for i in range(8)], True)
    _carve(x, exp, [(5 + i, 36) for i in range(9)], False)
    cases.append(("8 filled, 9 kept, borders and corners", x, 8, exp))
    # two 5-pixel pieces that touch only diagonally are ONE component of 10 (kept); two 4-pixel pieces make 8 (filled); both diagonals
    x = _plane(1, 24, 37)
    exp = x.copy()
    _carve(x, exp, [(2, 3 + j) for j in range(5)] + [(3, 8 + j) for j in range(5)], False)             # "\"
    _carve(x, exp, [(6, 8 + j) for j in range(5)] + [(7, 3 + j) for j in range(5)], False)             # "/"
    _carve(x, exp, [(10, 3 + j) for j in range(4)] + [(11, 7 + j) for j in range(4)], True)
    _carve(x, exp, [(14, 7 + j) for j in range(4)] + [(15, 3 + j) for j in range(4)], True)
    _carve(x, exp, [(19 + i, 20) for i in range(5)] + [(18 - i, 21 + i) for i in range(4)], False)    # a column of 5 and a "/" diagonal of 4 from its top: 9
    _carve(x, exp, [(2 + i, 25 + i) for i in range(8)], True)                                          # a pure "\\" diagonal of 8
    _carve(x, exp, [(12 + i, 36 - i) for i in range(9)], False)                                        # a pure "/" diagonal of 9
    cases.append(("diagonal contacts", x, 8, exp))
    # W = 130: runs across the 64-lane boundary of a row (lanes 60..67) and across the second one
    x = _plane(1, 9, 130)
    exp = x.copy()
    _carve(x, exp, [(1, c) for c in range(60, 68)], True)
    _carve(x, exp, [(3, c) for c in range(60, 69)], False)
    _carve(x, exp, [(5, c) for c in range(124, 130)], True)
    _carve(x, exp, [(7, c) for c in range(121, 130)], False)
    _carve(x, exp, [(5, c) for c in range(0, 3)] + [(4, 2), (6, 2)], True)
    cases.append(("runs across lane 63 | 64", x, 8, exp))
    # widths and one-row / one-column planes: runs of 3, 8 and 9, a run that ends at the row's end
    for W in (1, 37, 64, 70, 130, 256):
        for H in (1, 5):
            runs = [(0, 1)] if W == 1 else [(0, 3), (5, 9), (16, 8), (W - 8, 8)] if W >= 37 else []
            if W >= 130:
                runs += [(58, 9), (70, 8)]
            if W == 256:
                runs += [(120, 9), (180, 8), (190, 16)]
            x, exp = _rows(2, H, W, runs)
            cases.append((f"rows of runs, H {H} W {W}", x, 8, exp))
    x, exp = _rows(1, 1, 70, [(0, 3), (5, 9), (16, 8), (62, 8)])
    cases.append(("one-column plane", np.ascontiguousarray(x.transpose(0, 2, 1)), 8, np.ascontiguousarray(exp.transpose(0, 2, 1))))
    # all positive: unchanged; all non-positive: unchanged at 8, wholly filled at H * W
    x = _plane(2, 20, 37)
    cases.append(("all positive", x, 8, x.copy()))
    cases.append(("all non-positive, max_area 8", -x, 8, -x))
    cases.append(("all non-positive, max_area H * W", -x[:1], 20 * 37, np.full((1, 20, 37), FILL, np.float32)))
    cases.append(("all non-positive, max_area H * W - 1", -x[:1], 20 * 37 - 1, -x[:1]))
    # a plane whose whole background is 5 pixels
    x = _plane(1, 33, 70)
    exp = x.copy()
    _carve(x, exp, [(16, 30), (16, 31), (17, 32), (18, 31), (18, 30)], True)
    cases.append(("background of 5 pixels", x, 8, exp))
    # 0.0 and -0.0 are background, NaN is not (and separates two runs of 8)
    x = _plane(1, 12, 37)
    exp = x.copy()
    _carve(x, exp, [(1, 3)], True, value=0.0)
    _carve(x, exp, [(1, 7)], True, value=-0.0)
    x[0, 1, 11] = exp[0, 1, 11] = np.nan
    _carve(x, exp, [(3, c) for c in range(2, 10)], True)
    x[0, 3, 10] = exp[0, 3, 10] = np.nan
    _carve(x, exp, [(3, c) for c in range(11, 19)], True)
    _carve(x, exp, [(5, c) for c in range(2, 6)], True, value=0.0)
    _carve(x, exp, [(5, c) for c in range(6, 10)], True, value=-0.0)
    _carve(x, exp, [(7, c) for c in range(2, 7)], False, value=-0.0)
    _carve(x, exp, [(7, c) for c in range(7, 11)], False, value=0.0)
    x[0, 9, 5] = exp[0, 9, 5] = -np.nan
    x[0, 9, 7] = exp[0, 9, 7] = np.float32(1e-45)                                                      # the smallest denormal is positive
    _carve(x, exp, [(9, 9)], True, value=-1e-45)
    cases.append(("zeros, signed zeros and NaN", x, 8, exp))
    # three planes: 5 pixels in the last row of plane i directly above 5 pixels in the first row of plane i + 1 - two components
    x = _plane(3, 6, 37)
    exp = x.copy()
    for p in range(2):
        _carve(x, exp, [(5, 10 + j) for j in range(5)], True, plane=p)
        _carve(x, exp, [(0, 10 + j) for j in range(5)], True, plane=p + 1)
    _carve(x, exp, [(5, 32 + j) for j in range(5)], True, plane=0)                                     # a row's end and the next plane's first pixels
    _carve(x, exp, [(0, j) for j in range(5)], True, plane=1)
    cases.append(("planes do not leak", x, 8, exp))
    # a one-pixel-wide spiral of more than 1 000 pixels: one component, kept
    g, n = spiral()
    assert n > 1000
    cases.append(("spiral", g[None].copy(), 8, g[None].copy()))
    cases.append(("spiral, max_area its length", g[None].copy(), n, np.where(g[None] <= 0, FILL, g[None]).astype(np.float32)))
    cases.append(("spiral, max_area its length - 1", g[None].copy(), n - 1, g[None].copy()))
    return cases
