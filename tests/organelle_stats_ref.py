"""numpy fp64 restatement of the organelle-statistics loop (the semantics of saber.analysis.organelle_statistics.extract_organelle_statistics with
skimage.measure.regionprops behind it), written from the published definitions, plus scene builders and an O(N) route to the integer moments.

Per label > 0 (np.unique order), the whole label being ONE region, connected or not:
  n         voxel count; a label with n < 3 gets no coordinate and no row
  centroid  mean voxel coordinate (z, y, x); reversed to (x, y, z) with xyz_order
  C         covariance of the voxel coordinates about the centroid, divided by n (no Bessel correction)
  I         inertia tensor tr(C) Id - C; ev = its eigenvalues, descending, clipped at 0
  axis_major_length = sqrt(10 (ev0 + ev1 - ev2))      (= sqrt(20 lambda_max(C)))
  axis_minor_length = sqrt(10 (-ev0 + ev1 + ev2))     (= sqrt(20 lambda_min(C)); the argument is clamped at 0 here, see below)
  volume = n (voxel_size / 10)^3,  diameter = (axis_minor_length + axis_major_length) / 2 * (voxel_size / 10)
The reference's equivalent-sphere fall-back for a negative sqrt argument (flat labels, where rounding decides the sign) is a documented
deviation of saber_amd and is not restated: the argument is clamped at 0."""
import numpy as np

WORDS = ("n", "sz", "sy", "sx", "szz", "syy", "sxx", "szy", "szx", "syx", "zmin", "ymin", "xmin", "zmax", "ymax", "xmax")


# ---------------------------------------------------------------------------------------------- the restatement
def label_props(mask):
    """{label: dict(n, centroid (z,y,x), eig (eigenvalues of C, descending), major, minor, extent (z,y,x))} for every label > 0"""
    mask = np.asarray(mask)
    labels = np.unique(mask)
    labels = labels[labels > 0]
    out = {}
    for label in labels:
        P = np.stack(np.nonzero(mask == label), axis=1).astype(np.float64)
        n = P.shape[0]
        c = P.mean(axis=0)
        Q = P - c
        C = Q.T @ Q / n
        inertia = np.trace(C) * np.eye(3) - C
        ev = np.clip(np.sort(np.linalg.eigvalsh(inertia))[::-1], 0, None)
        major = np.sqrt(10 * (ev[0] + ev[1] - ev[2]))
        minor = np.sqrt(max(10 * (-ev[0] + ev[1] + ev[2]), 0.0))
        out[int(label)] = dict(n=n, centroid=c, eig=np.sort(np.linalg.eigvalsh(C))[::-1], major=float(major), minor=float(minor),
                               extent=tuple(int(v) for v in (P.max(axis=0) - P.min(axis=0) + 1)))
    return out


def expected(mask, run_name, voxel_size, xyz_order=True, props=None):
    """(coordinates {str(label): centroid tuple}, csv rows) as the reference loop leaves them"""
    props = label_props(mask) if props is None else props
    coordinates, rows = {}, []
    for label in sorted(props):
        p = props[label]
        if p["n"] < 3:
            continue
        c = tuple(float(v) for v in p["centroid"])
        coordinates[str(label)] = c[::-1] if xyz_order else c
        volume = p["n"] * (voxel_size / 10) ** 3
        diameter = (p["minor"] * (voxel_size / 10) + p["major"] * (voxel_size / 10)) / 2
        rows.append([run_name, int(label), volume, diameter])
    return coordinates, rows


def table_from_props(props):
    """the host table saber_amd.analysis.organelle_table returns, built from label_props (for tests that replace the device call)"""
    labels = sorted(props)
    return {"label": np.array(labels, np.int64), "count": np.array([props[v]["n"] for v in labels], np.int64),
            "centroid": np.array([props[v]["centroid"] for v in labels], np.float64).reshape(-1, 3),
            "bbox": np.zeros((len(labels), 6), np.int64),
            "axis_major_length": np.array([props[v]["major"] for v in labels], np.float64),
            "axis_minor_length": np.array([props[v]["minor"] for v in labels], np.float64),
            "eigenvalues": np.array([props[v]["eig"] for v in labels], np.float64).reshape(-1, 3)}


# ---------------------------------------------------------------------------------------------- O(N) integer moments
def moments(mask):
    """(labels ascending (K,) int64, moments (K,16) int64 in the order of WORDS) of every label > 0: np.bincount with integer-valued fp64
    weights, exact while every sum stays below 2^53 (asserted)."""
    mask = np.asarray(mask)
    Z, H, W = mask.shape
    idx = np.flatnonzero(mask.reshape(-1) > 0)
    if idx.size == 0:
        return np.zeros(0, np.int64), np.zeros((0, 16), np.int64)
    vals = mask.reshape(-1)[idx].astype(np.int64)
    labels, inv = np.unique(vals, return_inverse=True)
    K = labels.size
    x = idx % W
    y = (idx // W) % H
    z = idx // (W * H)
    out = np.zeros((K, 16), np.int64)
    out[:, 0] = np.bincount(inv, minlength=K)
    for j, w in enumerate((z, y, x, z * z, y * y, x * x, z * y, z * x, y * x), start=1):
        s = np.bincount(inv, weights=w.astype(np.float64), minlength=K)
        assert s.max() < 2.0 ** 53, "bincount route: a sum reached 2^53 and is no longer exact"
        out[:, j] = s.astype(np.int64)
    order = np.argsort(inv, kind="stable")
    starts = np.searchsorted(inv[order], np.arange(K))
    for j, w in enumerate((z, y, x)):
        out[:, 10 + j] = np.minimum.reduceat(w[order], starts)
        out[:, 13 + j] = np.maximum.reduceat(w[order], starts)
    return labels.astype(np.int64), out


# ---------------------------------------------------------------------------------------------- scenes
def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def ellipsoid(shape, centre, semi_axes, R):
    """solid ellipsoid: voxels p with |diag(1/semi_axes) R^T (p - centre)| <= 1 (coordinates in z, y, x order)"""
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), axis=-1) - np.asarray(centre, np.float64)
    u = (g @ R) / np.asarray(semi_axes, np.float64)
    return (u * u).sum(axis=-1) <= 1.0


def blob_scene(shape, seed, n_labels=12, dtype=np.int32, values=None):
    """random rotated solid ellipsoids with semi-axes >= 1.5 voxels, later blobs overwriting earlier ones, then a 2x2x2 cube at every blob's
    centre (so that a label survives with an extent of at least 2 voxels on every axis unless another cube lands on it); label values 1..n or
    `values`.  Needs Z, H, W >= 2."""
    rng = np.random.default_rng(seed)
    Z, H, W = shape
    vol = np.zeros(shape, np.int64)
    values = list(range(1, n_labels + 1)) if values is None else list(values)
    centres = []
    for v in values:
        c = np.array([rng.integers(0, max(Z - 1, 1)), rng.integers(0, max(H - 1, 1)), rng.integers(0, max(W - 1, 1))])
        ax = np.array([rng.uniform(1.5, max(2.0, Z / 3)), rng.uniform(1.5, max(2.0, H / 4)), rng.uniform(1.5, max(2.0, W / 4))])
        m = ellipsoid(shape, c, ax, rotation(rng))
        vol[m] = v
        centres.append(c)
    for v, c in zip(values, centres):
        vol[c[0]:c[0] + 2, c[1]:c[1] + 2, c[2]:c[2] + 2] = v
    return vol.astype(dtype)
