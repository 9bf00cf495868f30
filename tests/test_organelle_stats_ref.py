"""CPU: the numpy restatement of the organelle-statistics loop (tests/organelle_stats_ref.py) against the analytic identities it must
satisfy.  skimage and copick are not available to run the reference itself, so its arithmetic is pinned here and by the device tests."""
import numpy as np
import pytest

import organelle_stats_ref as ref


@pytest.mark.parametrize("semi", [(20, 12, 7), (9, 30, 14), (6, 6, 6)])
def test_rotated_solid_ellipsoid_gives_its_axes(semi):
    """a solid ellipsoid with semi-axes a >= b >= c has axis_major_length 2a and axis_minor_length 2c; the voxelisation error of semi-axes
    >= 6 was at most 0.8 % when this was written, 2 % is asserted"""
    rng = np.random.default_rng(sum(semi))
    shape = (72, 72, 72)
    centre = np.array([35.3, 36.1, 34.8])
    vol = ref.ellipsoid(shape, centre, semi, ref.rotation(rng)).astype(np.int32) * 5
    p = ref.label_props(vol)[5]
    a, c = max(semi), min(semi)
    print(f"semi-axes {semi}: major {p['major']:.4f} (2a = {2 * a}), minor {p['minor']:.4f} (2c = {2 * c})")
    assert abs(p["major"] - 2 * a) <= 0.02 * 2 * a
    assert abs(p["minor"] - 2 * c) <= 0.02 * 2 * c
    assert np.abs(p["centroid"] - centre).max() <= 0.5
    # sqrt(10 (ev0 + ev1 - ev2)) on the inertia tensor is sqrt(20 lambda_max(C)), and likewise for the minor length
    assert p["major"] == pytest.approx(np.sqrt(20 * p["eig"][0]), rel=1e-12)
    assert p["minor"] == pytest.approx(np.sqrt(20 * p["eig"][2]), rel=1e-12)


def test_skip_rule_background_rule_and_xyz_order():
    vol = np.zeros((6, 8, 10), np.int16)
    vol[1, 2, 3:5] = 4                      # 2 voxels: skipped
    vol[2:4, 1:4, 5:9] = 7                  # 24 voxels
    vol[5, 7, 7:10] = 9                     # exactly 3 voxels: kept
    vol[0, 0, 0:5] = -3                     # negative: background
    props = ref.label_props(vol)
    assert sorted(props) == [4, 7, 9]
    coords, rows = ref.expected(vol, "run_a", 10.0)
    assert list(coords) == ["7", "9"] and [r[1] for r in rows] == [7, 9]
    assert coords["7"] == pytest.approx((6.5, 2.0, 2.5))                      # (x, y, z)
    coords_zyx, _ = ref.expected(vol, "run_a", 10.0, xyz_order=False)
    assert coords_zyx["7"] == pytest.approx((2.5, 2.0, 6.5))
    assert rows[0][0] == "run_a" and rows[0][2] == pytest.approx(24.0)        # voxel_size 10 A = 1 nm
    _, rows5 = ref.expected(vol, "run_a", 5.0)
    assert rows5[0][2] == pytest.approx(24 * 0.125) and rows5[0][3] == pytest.approx(rows[0][3] / 2)
    # a line has no extent across: minor length 0 (clamped), major = sqrt(20 var) with var = 2/3 for 3 voxels
    assert props[9]["minor"] == pytest.approx(0.0, abs=1e-6) and props[9]["major"] == pytest.approx(np.sqrt(20 * 2 / 3))


def test_disconnected_label_is_one_region():
    vol = np.zeros((4, 10, 30), np.uint8)
    vol[1:3, 2:4, 2:4] = 3
    vol[1:3, 2:4, 22:24] = 3
    p = ref.label_props(vol)[3]
    assert p["n"] == 16 and p["centroid"] == pytest.approx((1.5, 2.5, 12.5)) and p["extent"] == (2, 2, 22)


def test_moment_route_reproduces_the_restatement():
    vol = ref.blob_scene((12, 40, 70), 3, n_labels=9)
    labels, mom = ref.moments(vol)
    props = ref.label_props(vol)
    assert labels.tolist() == sorted(props)
    for k, v in enumerate(labels.tolist()):
        n = mom[k, 0]
        assert n == props[v]["n"]
        assert mom[k, 1:4] / n == pytest.approx(props[v]["centroid"], abs=1e-9)
        assert tuple(mom[k, 13:16] - mom[k, 10:13] + 1) == props[v]["extent"]
        S, M = mom[k, 1:4].astype(np.float64), np.array([[mom[k, 4], mom[k, 7], mom[k, 8]], [mom[k, 7], mom[k, 5], mom[k, 9]],
                                                         [mom[k, 8], mom[k, 9], mom[k, 6]]], np.float64)
        C = M / n - np.outer(S, S) / n ** 2
        assert np.sort(np.linalg.eigvalsh(C))[::-1] == pytest.approx(props[v]["eig"], rel=1e-9, abs=1e-9)
    assert ref.moments(np.zeros((2, 3, 4), np.int32))[1].shape == (0, 16)
