"""The volumes whose smoothed bytes tests/golden/smooth_parent_bits.npz pins (tests/test_gpu_smooth_parent_bits.py; recorded by
tools/record_smooth_bits.py).  Everything is rebuilt from seeds: the fixture holds outputs only."""
import numpy as np

import sharded_smooth_ref as ref

FIELD_SIGMA = 1.5


def _block(vol, label, z, y, x, rng):
    """`label` on the box z x y x x (inclusive ranges) with 10 % of its voxels knocked out; the eight corners stay, so the box is the label's"""
    sub = vol[z[0]:z[1] + 1, y[0]:y[1] + 1, x[0]:x[1] + 1]
    keep = rng.uniform(size=sub.shape) < 0.9
    for c in np.ndindex(2, 2, 2):
        keep[tuple(-i for i in c)] = True
    sub[keep] = label


def deep():
    """(40,12,70): label 1 on the planes 3..38 - a box of 36 planes, deeper than the z tile of 32, starting above plane 0 - and a small
    label 2; radius 9 / 2 at scale 0.1, so from 2 chunks on a chunk's own planes start inside label 1's box"""
    rng = np.random.default_rng(7)
    vol = np.zeros((40, 12, 70), np.int32)
    _block(vol, 1, (3, 38), (2, 9), (5, 60), rng)
    _block(vol, 2, (10, 13), (1, 4), (63, 68), rng)
    return vol, 0.1


def edges():
    """(6,40,140): boxes of dx = 64, 65 and 1, dy = 33, 32 and 33, dz * dy = 165, 192 and 99: the last x tile full, one column into the
    next, a single column; the y tile full and one row over; dead rows in the last 4-row block of the x pass"""
    rng = np.random.default_rng(8)
    vol = np.zeros((6, 40, 140), np.int32)
    _block(vol, 1, (0, 4), (2, 34), (3, 66), rng)
    _block(vol, 2, (0, 5), (4, 35), (70, 134), rng)
    _block(vol, 3, (1, 3), (5, 37), (138, 138), rng)
    return vol, 0.1


def label_cases():
    """name -> (volume, scale) of the label volumes"""
    return {"blob_a": ref.blob_case("a"), "blob_b": ref.blob_case("b"), "deep": deep(), "edges": edges()}


def field_mask():
    """the 0/1 mask whose float field is pinned (sigma FIELD_SIGMA)"""
    return (ref.blob_case("a")[0] != 0).astype(np.uint8)
