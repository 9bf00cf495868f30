"""The sharded smoothing scheme (saber_amd/segmenters/smooth.py, csrc/smooth3d.hip: saber_smooth_labels_chunk) restated in numpy on top of
the oracle's separable filter (oracle.saber_ref.gaussian_smoothing_3d), and the test volumes the host and the GPU tests share.

Per chunk [z0, z1) of the volume: every label's count comes from the WHOLE volume, the chunk sees the planes [z0 - h, z1 + h) clipped to
the volume (h = the largest radius of any label), a label is filtered on the planes [z0 - r, z1 + r) only, and it is skipped when its
voxels there all lie on one side of the own planes.  `naive_skip` replaces that rule by "no voxel in the own planes": wrong, see
sandwich()."""
import numpy as np

from oracle import saber_ref


def sigma_of(count: int, scale: float) -> float:
    """the oracle's sigma of a mask of `count` voxels (it only sums the mask)"""
    return saber_ref.estimate_feature_size_3d(np.array([int(count)]), scale)


def radius_of(count: int, scale: float) -> int:
    return len(saber_ref.gaussian_taps_3d(sigma_of(count, scale))) // 2


def cuts_of(Z: int, parts: int):
    """the split of tests/test_gpu_sharded_stitch.py: `parts` consecutive chunks"""
    c = [round(i * Z / parts) for i in range(parts + 1)]
    return list(zip(c[:-1], c[1:]))


def smooth_chunks_ref(volume: np.ndarray, bounds, scale: float, naive_skip: bool = False) -> np.ndarray:
    """fast_3d_gaussian_smoothing of `volume`, chunk by chunk.  bounds: [(z0, z1)] consecutive chunks (empty ones allowed)."""
    Z = volume.shape[0]
    counts = np.bincount(volume.ravel())
    ids = np.flatnonzero(counts[1:]) + 1
    h = max([radius_of(counts[v], scale) for v in ids] + [0])
    out = np.zeros(volume.shape, np.uint8)
    for z0, z1 in bounds:
        if z1 <= z0:
            continue
        e0, e1 = max(z0 - h, 0), min(z1 + h, Z)                    # what the chunk holds: its planes and the two halos
        for v in np.unique(volume[e0:e1]):
            if v == 0:
                continue
            sigma = sigma_of(counts[v], scale)
            r = radius_of(counts[v], scale)
            w0, w1 = max(z0 - r, e0), min(z1 + r, e1)
            m = volume[w0:w1] == v
            zs = np.flatnonzero(m.any(axis=(1, 2))) + w0
            if naive_skip:
                skip = not ((zs >= z0) & (zs < z1)).any()
            else:
                skip = zs.size == 0 or zs.max() < z0 or zs.min() >= z1
            if skip:
                continue
            field = saber_ref.gaussian_smoothing_3d(m, sigma)[z0 - w0: z1 - w0]
            out[z0:z1][field > 0.5] = np.uint8(int(v) & 255)
    return out


def blobs(shape, n, seed, rmin, rmax, dtype=np.uint32):
    """the blob recipe of tests/test_gpu_smooth3d.py: n ellipsoids with 10 % of their voxels knocked out, labels 1..n"""
    rng = np.random.default_rng(seed)
    Z, H, W = shape
    vol = np.zeros(shape, dtype)
    zz, yy, xx = np.mgrid[:Z, :H, :W]
    for k in range(n):
        cz, cy, cx = rng.integers(0, Z), rng.integers(0, H), rng.integers(0, W)
        rz, ry, rx = rng.uniform(rmin, rmax, 3)
        m = ((zz - cz) / rz) ** 2 + ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
        m &= rng.uniform(size=shape) < 0.9
        vol[m] = k + 1
    return vol


def blob_case(name: str):
    """(volume uint32, scale) of the named blob volume; "a" and "b" carry label values above 255 and above 65535"""
    if name == "a":
        vol, scale = blobs((12, 40, 70), 14, seed=54, rmin=2.0, rmax=9.0), 0.15
    elif name == "b":
        vol, scale = blobs((9, 33, 65), 10, seed=43, rmin=2.0, rmax=8.0), 0.3
    else:
        return blobs((20, 150, 333), 40, seed=190, rmin=2.0, rmax=20.0), 0.075      # test_blobs_match_oracle's first case
    vol[vol == 3] = 300
    vol[vol == 5] = 70000
    vol[vol == 6] = 65536 + 6                                       # the same byte as label 6 would give: modulo 256
    return vol, scale


def sandwich():
    """label 7 on the planes 0-3 and 5-8, none on plane 4: at scale 0.15 (radius 8) the whole-volume filter sets 304 voxels of plane 4"""
    vol = np.zeros((9, 30, 40), np.uint32)
    vol[0:4, 5:25, 8:28] = 7
    vol[5:9, 5:25, 8:28] = 7
    return vol, 0.15
