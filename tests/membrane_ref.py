"""Test helper: the organelle / membrane refinement pipeline restated in numpy + scipy.ndimage.

Written from the observed behaviour of saber.analysis.refine_membranes.OrganelleMembraneFilter ("membrane
refinement"), not from its text: binary_dilation / binary_erosion with an explicit ball and a zero border, 6-connected
scipy.ndimage.label.  Everything is integer or boolean work, so the device pipeline must agree bit for bit.

    pairs, n_labels_in = refine(org, mem, ball_size=3, ...)
    pairs: [(label_out, (z0, y0, x0, z1, y1, x1), org_roi bool, mem_roi bool)], ascending label; label_out = label + 1
    flatten(pairs, shape, dtype) -> the two 3-D label maps;  stacks(pairs, shape, dtype) -> the two 4-D stacks
"""
import numpy as np
import scipy.ndimage as ndi


def ball(r: int) -> np.ndarray:
    g = np.arange(-r, r + 1)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return (z * z + y * y + x * x) <= r * r


def dilate(m, r):
    return ndi.binary_dilation(m, structure=ball(r)) if m.any() else m.copy()


def erode(m, r):
    return ndi.binary_erosion(m, structure=ball(r)) if m.any() else m.copy()        # border_value = 0: the outside erodes the edge


def opening(m, r):
    return dilate(erode(m, r), r)


def drop_small(m, min_size):
    lab, n = ndi.label(m)                                   # default structure: 6-connectivity
    if n == 0:
        return np.zeros_like(m)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    keep = sizes >= min_size
    keep[0] = False
    return keep[lab]


def largest(m):
    lab, n = ndi.label(m)
    if n == 0:
        return np.zeros_like(m)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    return lab == (int(np.argmax(sizes)) + 1)               # argmax: the first of the largest, in scipy's raster label order


def surface_only(mem, org):
    """components of `mem` with more than a tenth of their voxels on the organelle's boundary (organelle minus its 3x3x3 erosion)"""
    boundary = org & ~ndi.binary_erosion(org, structure=np.ones((3, 3, 3), bool))
    lab, n = ndi.label(mem)
    if n == 0:
        return mem.copy()
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    on = np.bincount(lab[boundary].ravel(), minlength=n + 1)
    keep = on * 10 > sizes                                   # on / size > 0.1 in integers
    keep[0] = False
    return keep[lab]


def trim(m, tz, txy):
    out = np.zeros_like(m)
    Z, H, W = m.shape
    if not (0 < tz < Z // 2):                                # m[0:-0] is empty: a zero trim leaves nothing
        return out
    if not (0 < txy < H // 2 and txy < W // 2):
        return out
    out[tz:Z - tz, txy:H - txy, txy:W - txy] = m[tz:Z - tz, txy:H - txy, txy:W - txy]
    return out


def roi_thresholds(shape, min_roi_relative_size):
    return np.float32(min_roi_relative_size) * np.asarray(shape, np.float32)


def refine(org, mem, ball_size=3, min_membrane_area=10000, edge_trim_z=5, edge_trim_xy=3, min_roi_relative_size=0.15,
           keep_surface_membranes=False, only_labels=None, **_):
    org = np.asarray(org)
    shape = org.shape
    mem_clean = drop_small(trim(np.asarray(mem) != 0, edge_trim_z, edge_trim_xy), min_membrane_area)
    zpres = mem_clean.any(axis=(1, 2))
    orgf = org * zpres[:, None, None].astype(org.dtype)
    labels = [int(v) for v in np.unique(orgf) if v > 0]
    thr = roi_thresholds(shape, min_roi_relative_size)
    pad = ball_size // 2
    pairs = []
    for v in labels:
        if only_labels is not None and v not in only_labels:
            continue
        sl = ndi.find_objects((orgf == v).astype(np.uint8))[0]
        lo = np.array([s.start for s in sl])
        hi = np.array([s.stop for s in sl])
        if ((hi - lo).astype(np.float32) < thr).any():
            continue
        lo = np.maximum(lo - pad, 0)
        hi = np.minimum(hi + pad, shape)
        box = tuple(slice(a, b) for a, b in zip(lo, hi))
        o = orgf[box] == v
        m = mem_clean[box]
        ext = hi - lo
        if ext.max() > 3 * ext.min():
            r_dil, r_open = 1, max(1, ball_size // 2)
        else:
            r_dil, r_open = 2, ball_size
        enhanced = dilate(m, r_dil) & dilate(o, r_dil)
        cleaned = drop_small(enhanced, 100)
        if keep_surface_membranes:
            cleaned = surface_only(cleaned, o)
        if not cleaned.any():
            continue
        combined = o | cleaned
        opened = opening(combined, r_open)
        if not opened.any():
            opened = combined
        opened = largest(opened)
        o_out = largest(o & opened)
        m_out = drop_small(cleaned & opened, 50)
        pairs.append((v + 1, tuple(int(a) for a in lo) + tuple(int(b) for b in hi), o_out, m_out))
    return pairs, len(labels)


def flatten(pairs, shape, dtype=np.uint8):
    o3, m3 = np.zeros(shape, dtype), np.zeros(shape, dtype)
    for v, (z0, y0, x0, z1, y1, x1), o, m in pairs:
        o3[z0:z1, y0:y1, x0:x1][o] = v
        m3[z0:z1, y0:y1, x0:x1][m] = v
    return o3, m3


def stacks(pairs, shape, dtype=np.uint8):
    o4, m4 = np.zeros((len(pairs),) + tuple(shape), dtype), np.zeros((len(pairs),) + tuple(shape), dtype)
    for k, (v, (z0, y0, x0, z1, y1, x1), o, m) in enumerate(pairs):
        o4[k, z0:z1, y0:y1, x0:x1][o] = v
        m4[k, z0:z1, y0:y1, x0:x1][m] = v
    return o4, m4


# ---- seeded scenes for the larger GPU comparisons (the committed fixture's scenes are built by tools/make_golden_membranes.py)
def ellipsoid(shape, c, r):
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0


def random_scene(shape, n_labels, seed, dtype=np.int32, shell=(1.0, 2.0), r_lo=0.08, r_hi=0.22, membrane_fraction=0.8):
    """n_labels ellipsoids (later ones overwrite earlier ones) and a membrane volume of shells around most of them, plus specks"""
    rng = np.random.default_rng(seed)
    org = np.zeros(shape, dtype)
    mem = np.zeros(shape, np.uint8)
    sh = np.array(shape, np.float64)
    for v in range(1, n_labels + 1):
        r = np.maximum(rng.uniform(r_lo, r_hi, 3) * sh, 3.0)
        c = rng.uniform(0.1, 0.9, 3) * sh
        lo = np.maximum(np.floor(c - r - shell[0] - 2).astype(int), 0)
        hi = np.minimum(np.ceil(c + r + shell[0] + 3).astype(int), shape)
        box = tuple(slice(a, b) for a, b in zip(lo, hi))
        sub = tuple(b - a for a, b in zip(lo, hi))
        org[box][ellipsoid(sub, c - lo, r)] = v
        if rng.uniform() < membrane_fraction:
            outer = ellipsoid(sub, c - lo, r + shell[0])
            inner = ellipsoid(sub, c - lo, np.maximum(r - shell[1], 0.5))
            mem[box][outer & ~inner] = 1
    mem[rng.uniform(size=shape) < 0.002] = 1
    return org, mem
