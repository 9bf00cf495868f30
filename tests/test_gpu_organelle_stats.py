"""GPU: csrc/labelstats.hip (label compaction, one-pass integer moments, fp64 finalise) and saber_amd.analysis.organelle_statistics on top of
it.  The integer tables are compared with the numpy O(N) route of tests/organelle_stats_ref.py by exact equality; the derived fp64
quantities with the numpy restatement of the reference loop within bounds that come from fp64 rounding on exact numerators plus the
backward error of Jacobi and LAPACK, with three orders of margin: eigenvalues 1e-12 * lambda_max, centroids 1e-9 voxel, axis lengths and
diameter 1e-9 relative on labels that extend over at least 2 voxels on every axis."""
import os
import time

import numpy as np
import pytest
import torch

import membrane_ref
import organelle_stats_ref as ref

pytestmark = pytest.mark.gpu
TIMING_LINES = {}


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    from saber_amd.filters._context import handle
    return handle(0)


def write_timing_file():
    out_dir = os.environ.get("SABER_AMD_TIMING_DIR", "timing_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "organelle_stats_timing.txt"), "w") as fh:
        for key in sorted(TIMING_LINES):
            fh.write(TIMING_LINES[key] + "\n")


def device_tables(ctx, vol, **kw):
    """(labels (K,) int64, moments (K,16) int64, stats (K,8) float64) of a numpy or device volume, on the host"""
    t = torch.from_numpy(np.ascontiguousarray(vol)).cuda() if isinstance(vol, np.ndarray) else vol
    labels, mom, stats = ctx.label_statistics(t, **kw)
    return labels.cpu().numpy().astype(np.int64), mom.cpu().numpy(), stats.cpu().numpy()


def assert_exact(ctx, vol, **kw):
    labels, mom, stats = device_tables(ctx, vol, **kw)
    want_labels, want_mom = ref.moments(vol if isinstance(vol, np.ndarray) else vol.cpu().numpy())
    assert labels.tolist() == want_labels.tolist()
    assert mom.shape == want_mom.shape
    bad = np.argwhere(mom != want_mom)
    assert bad.size == 0, f"first differing (row, word): {bad[0].tolist()} label {labels[bad[0][0]]} {ref.WORDS[bad[0][1]]}: " \
                          f"{mom[tuple(bad[0])]} != {want_mom[tuple(bad[0])]}"
    return labels, mom, stats


# ---------------------------------------------------------------------------------------------- exact integers
@pytest.mark.parametrize("shape", [(12, 40, 70), (5, 9, 40), (6, 33, 515), (3, 20, 1030), (16, 64, 512), (2, 2, 2), (40, 70, 9)])
def test_moments_equal_the_numpy_route(ctx, shape):
    vol = ref.blob_scene(shape, sum(shape), n_labels=10)
    assert_exact(ctx, vol)
    assert_exact(ctx, vol, per_piece_atomics=True)                          # the baseline form of the kernel computes the same table
    assert_exact(ctx, vol, capacity=1)                                      # the capacity is found on the second try


def test_three_calls_are_bit_identical(ctx):
    vol = torch.from_numpy(ref.blob_scene((24, 96, 600), 5, n_labels=40)).cuda()
    first = ctx.label_statistics(vol)
    for _ in range(2):
        again = ctx.label_statistics(vol)
        for a, b in zip(first, again):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                                      b.view(torch.int64) if b.dtype == torch.float64 else b)
    assert first[0].numel() >= 20


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16, np.int32, np.uint32])
def test_every_device_dtype(ctx, dtype):
    vol = ref.blob_scene((8, 30, 100), 11, n_labels=12, dtype=dtype)
    if np.issubdtype(dtype, np.signedinteger):
        vol[0, :, 0:7] = -5                                                 # negative values are background
        vol[7, 3, :] = np.iinfo(dtype).min
    labels, _, _ = assert_exact(ctx, vol)
    assert labels.size >= 8 and labels.min() > 0


def test_bool_and_int64_input_through_the_table(ctx):
    from saber_amd.analysis import organelle_table
    vol = ref.blob_scene((8, 30, 100), 12, n_labels=12, dtype=np.int64)
    vol[0, 0, :] = -(2 ** 40) + 7                                           # would alias a small positive value if it were truncated
    for v in (vol, torch.from_numpy(vol), torch.from_numpy(vol).cuda(), vol > 0, torch.from_numpy(vol > 0).cuda(), vol.astype(np.int8)):
        host = v.cpu().numpy() if isinstance(v, torch.Tensor) else v
        want_labels, want_mom = ref.moments(host.astype(np.int64))
        t = organelle_table(v)
        assert t["label"].tolist() == want_labels.tolist()
        assert np.array_equal(t["count"], want_mom[:, 0]) and np.array_equal(t["bbox"], want_mom[:, 10:16])
        assert np.allclose(t["centroid"], want_mom[:, 1:4] / want_mom[:, :1], rtol=0, atol=1e-9)
    with pytest.raises(ValueError, match="2\\^22"):
        organelle_table(np.full((2, 2, 2), 2 ** 22 + 1, np.int64))


def test_a_device_tensor_is_used_in_place(ctx):
    from saber_amd.analysis.organelle_statistics import _to_device
    vol = torch.from_numpy(ref.blob_scene((8, 30, 100), 13)).cuda()
    assert _to_device(vol, ctx.device).data_ptr() == vol.data_ptr()


def test_sparse_label_values(ctx):
    big = (1, 31, 32, 33, 65535, 65536, 4000000, 2 ** 22 - 1, 2 ** 22)
    for dtype in (np.int32, np.uint32):
        labels, _, _ = assert_exact(ctx, ref.blob_scene((10, 40, 90), 21, dtype=dtype, values=big))
        assert labels.max() == 2 ** 22 and labels.size >= 7
    labels, _, _ = assert_exact(ctx, ref.blob_scene((10, 40, 90), 22, dtype=np.uint16, values=(1, 255, 256, 32767, 32768, 65534, 65535)))
    assert labels.max() == 65535
    labels, _, _ = assert_exact(ctx, ref.blob_scene((10, 40, 90), 23, dtype=np.int16, values=(1, 2, 16384, 32766, 32767)))
    assert labels.max() == 32767
    labels, _, _ = assert_exact(ctx, ref.blob_scene((10, 40, 90), 24, dtype=np.uint8, values=(1, 127, 128, 254, 255)))
    assert labels.max() == 255
    over = np.zeros((2, 3, 4), np.uint32)
    over[1, 2, 3] = 2 ** 22 + 1
    with pytest.raises(ValueError, match="2\\^22"):
        ctx.label_statistics(torch.from_numpy(over).cuda())
    over[1, 2, 3] = 2 ** 22
    assert device_tables(ctx, over)[0].tolist() == [2 ** 22]


def test_special_scenes(ctx):
    Z, H, W = 7, 19, 75
    # empty volume: K = 0
    labels, mom, stats = device_tables(ctx, np.zeros((Z, H, W), np.int32))
    assert labels.shape == (0,) and mom.shape == (0, 16) and stats.shape == (0, 8)
    # a disconnected label is one region
    vol = np.zeros((Z, H, W), np.uint16)
    vol[1:3, 2:4, 2:4] = 3
    vol[5:7, 15:19, 70:75] = 3
    vol[3, 9, 30:40] = 8
    labels, mom, _ = assert_exact(ctx, vol)
    assert labels.tolist() == [3, 8] and mom[0, 0] == 8 + 40 and mom[0, 10:16].tolist() == [1, 2, 2, 6, 18, 74]
    # labels that touch every face: the whole volume, and a frame around another label
    assert_exact(ctx, np.full((Z, H, W), 6, np.uint8))
    vol = np.full((Z, H, W), 2, np.int32)
    vol[1:-1, 1:-1, 1:-1] = 9
    assert_exact(ctx, vol)
    # single-voxel labels, in the first and in the last voxel and in between
    vol = np.zeros((Z, H, W), np.int32)
    vol[0, 0, 0], vol[Z - 1, H - 1, W - 1], vol[3, 4, 64] = 5, 4, 100
    labels, mom, stats = assert_exact(ctx, vol)
    assert labels.tolist() == [4, 5, 100] and mom[:, 0].tolist() == [1, 1, 1]
    assert np.array_equal(stats[:, 0:3], np.array([[Z - 1, H - 1, W - 1], [0, 0, 0], [3, 4, 64]], np.float64)) and np.all(stats[:, 3:] == 0)


def test_bad_arguments(ctx):
    vol = torch.zeros((2, 3, 4), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="unsupported label dtype"):
        ctx.label_statistics(vol.to(torch.int64))
    import ctypes as C
    n = C.c_int(-1)
    lib, p = ctx.lib, C.c_void_p(vol.data_ptr())
    assert lib.saber_label_statistics(ctx.h, p, 4, 1, 2, 3, 70000, 0, 0, None, None, None, C.byref(n), None) == -1
    assert b"65535" in lib.saber_last_error(ctx.h)
    assert lib.saber_label_statistics(ctx.h, p, 4, 1, 2048, 1024, 1024, 0, 0, None, None, None, C.byref(n), None) == -1
    assert b"2^31" in lib.saber_last_error(ctx.h)
    assert lib.saber_label_statistics(ctx.h, p, 3, 0, 2, 3, 4, 0, 0, None, None, None, C.byref(n), None) == -1
    assert lib.saber_label_statistics(ctx.h, p, 1, 1, 2, 3, 4, 0, 0, None, None, None, C.byref(n), None) == -1
    assert lib.saber_label_statistics(ctx.h, p, 4, 1, 2, 3, 4, 0, 2, None, None, None, C.byref(n), None) == -1
    # a capacity that is too small is an error that names the needed K and writes nothing
    vol[0, 0, 0], vol[1, 2, 3], vol[1, 1, 1] = 7, 9, 8
    torch.cuda.synchronize()
    assert lib.saber_label_statistics(ctx.h, p, 4, 1, 2, 3, 4, 2, 0, None, None, None, C.byref(n), None) == -4
    assert n.value == 3 and b"holds 3 labels" in lib.saber_last_error(ctx.h) and b"room for 2" in lib.saber_last_error(ctx.h)


# ---------------------------------------------------------------------------------------------- derived quantities
def compare_with_restatement(labels, mom, stats, props, worst, lengths=True):
    """all labels: eigenvalues and centroids; labels of extent >= 2 on every axis: both lengths and the diameter (not for the scene of
    degenerate labels, lengths=False: a slanted line has an extent on every axis and no thickness).  Returns that count."""
    assert labels.tolist() == sorted(props)
    thick = 0
    for k, v in enumerate(labels.tolist()):
        p = props[v]
        assert mom[k, 0] == p["n"]
        lam_max = max(p["eig"][0], 1e-300)
        e_eig = np.abs(stats[k, 5:8] - p["eig"]).max() / lam_max
        e_cen = np.abs(stats[k, 0:3] - p["centroid"]).max()
        worst["eig"], worst["centroid"] = max(worst["eig"], e_eig), max(worst["centroid"], e_cen)
        assert e_eig <= 1e-12, (v, stats[k, 5:8], p["eig"])
        assert e_cen <= 1e-9, (v, stats[k, 0:3], p["centroid"])
        assert np.isfinite(stats[k]).all() and stats[k, 4] >= 0 and stats[k, 3] >= stats[k, 4]
        if lengths and min(p["extent"]) >= 2:
            thick += 1
            e_major, e_minor = abs(stats[k, 3] - p["major"]) / p["major"], abs(stats[k, 4] - p["minor"]) / p["minor"]
            d_dev, d_ref = (stats[k, 3] + stats[k, 4]) / 2 * 1.35, (p["major"] + p["minor"]) / 2 * 1.35
            worst["major"], worst["minor"] = max(worst["major"], e_major), max(worst["minor"], e_minor)
            worst["diameter"] = max(worst["diameter"], abs(d_dev - d_ref) / d_ref)
            assert e_major <= 1e-9 and e_minor <= 1e-9 and abs(d_dev - d_ref) <= 1e-9 * d_ref, (v, stats[k], p)
    return thick


def test_derived_quantities_against_the_restatement(ctx):
    worst = dict(eig=0.0, centroid=0.0, major=0.0, minor=0.0, diameter=0.0)
    n_labels = 0
    for shape, seed, dtype in (((12, 40, 70), 31, np.int32), ((5, 9, 40), 32, np.uint8), ((24, 96, 300), 33, np.uint16), ((6, 33, 515), 34, np.int16),
                               ((30, 200, 130), 35, np.uint32)):
        vol = ref.blob_scene(shape, seed, n_labels=14, dtype=dtype)
        props = ref.label_props(vol)
        labels, mom, stats = device_tables(ctx, vol)
        thick = compare_with_restatement(labels, mom, stats, props, worst)
        assert thick == len(props) and len(props) >= 8          # every label of a blob scene is compared in full
        n_labels += thick
    # rotated solid ellipsoids: the analytic identity (major 2a, minor 2c within the 2 % voxelisation bound of the CPU test)
    rng = np.random.default_rng(36)
    vol = np.zeros((72, 72, 72), np.int32)
    vol[ref.ellipsoid(vol.shape, (35.3, 36.1, 34.8), (20, 12, 7), ref.rotation(rng))] = 3
    labels, mom, stats = device_tables(ctx, vol)
    assert abs(stats[0, 3] - 40) <= 0.02 * 40 and abs(stats[0, 4] - 14) <= 0.02 * 14
    compare_with_restatement(labels, mom, stats, ref.label_props(vol), worst)
    # flat and line labels, built on purpose: count and centroid agree, the minor length is finite and >= 0
    vol = np.zeros((9, 40, 70), np.int32)
    zz, yy, xx = np.mgrid[:9, :40, :70]
    vol[(zz == 4) & ((yy - 20) ** 2 + (xx - 30) ** 2 < 150)] = 1           # a disc in one z plane
    vol[:, 7, :][(zz[:, 7, :] - 4) ** 2 + (xx[:, 7, :] - 50) ** 2 < 12] = 2  # a disc in one y plane
    vol[2:8, 30:38, 66] = 3                                                 # a patch in one x plane
    vol[1, 2, 3:60] = 4                                                     # a line along x
    vol[0:9, 39, 0] = 5                                                     # a line along z
    for i in range(9):
        vol[i, 25 + i, 5 + 2 * i] = 6                                       # a slanted line
    vol[8, 0, 69] = 7                                                       # one voxel
    vol[8, 0, 0:2] = 8                                                      # two voxels
    props = ref.label_props(vol)
    labels, mom, stats = assert_exact(ctx, vol)
    flat_worst = dict(worst)
    assert compare_with_restatement(labels, mom, stats, props, flat_worst, lengths=False) == 0 and len(props) == 8
    assert sum(min(p["extent"]) >= 2 for p in props.values()) == 1           # the slanted line alone
    assert np.isfinite(stats[:, 4]).all() and (stats[:, 4] >= 0).all()
    assert stats[:, 4].max() < 1e-3                                         # sqrt(20 * rounding error of an eigenvalue that is 0)
    worst["eig"], worst["centroid"] = flat_worst["eig"], flat_worst["centroid"]
    line = (f"derived quantities, worst over {n_labels} blob labels + 1 ellipsoid (eigenvalues / centroids also over 8 flat and line labels): "
            f"eigenvalues {worst['eig']:.2e} of lambda_max (bound 1e-12), centroid {worst['centroid']:.2e} voxel (1e-9), axis_major_length "
            f"{worst['major']:.2e}, axis_minor_length {worst['minor']:.2e}, diameter {worst['diameter']:.2e} relative (1e-9)")
    print("\n" + line)
    TIMING_LINES["1 accuracy"] = line
    write_timing_file()


# ---------------------------------------------------------------------------------------------- end to end
class Run:
    def __init__(self, name):
        self.name, self.picks = name, []


def check_extract(vol, voxel_size, capsys, **kw):
    from saber_amd.analysis import extract_organelle_statistics
    run, got = Run("run_7"), []
    rows = extract_organelle_statistics(run, vol, "mito", "1", "SABER", voxel_size, True, True,
                                        write_picks=lambda r, p, o, **k: got.append((p, o, k)), **kw)
    host = vol.cpu().numpy() if isinstance(vol, torch.Tensor) else vol
    coords, want = ref.expected(host, "run_7", voxel_size, **{k: v for k, v in kw.items() if k == "xyz_order"})
    assert [r[:2] for r in rows] == [r[:2] for r in want] and len(rows) >= 3
    assert [r[2] for r in rows] == [r[2] for r in want]                     # n * (voxel_size / 10)^3: the same arithmetic on the same integer
    assert np.allclose([r[3] for r in rows], [r[3] for r in want], rtol=1e-9, atol=0)
    (points, orientations, k), = got
    assert k == dict(object_name="mito", session_id="1", user_id="SABER")
    assert np.allclose(points, np.array(list(coords.values())) * voxel_size, rtol=0, atol=1e-9 * voxel_size)
    assert orientations.shape == (len(coords), 4, 4) and all(np.array_equal(o, np.eye(4)) for o in orientations)
    return rows, capsys.readouterr().out


def test_extract_on_device_tensor_and_numpy(ctx, capsys):
    vol = ref.blob_scene((14, 60, 90), 41, n_labels=9, dtype=np.uint16)
    vol[0, 0, 0:2] = 300                                                    # two voxels: skipped
    rows_np, out = check_extract(vol, 13.48, capsys)
    assert "Skipping label 300 in run_7: too small (< 3 voxels)" in out
    rows_dev, _ = check_extract(torch.from_numpy(vol).cuda(), 13.48, capsys)
    assert rows_dev == rows_np
    check_extract(torch.from_numpy(vol).cuda(), 10.0, capsys, xyz_order=False)
    from saber_amd.analysis import extract_organelle_statistics
    run = Run("run_0")
    assert extract_organelle_statistics(run, np.zeros((4, 5, 6), np.uint8), "mito", "1", "SABER", 10.0, write_picks=lambda *a, **k: 1 / 0) == []
    assert "run_0 didn't have any organelles present!" in capsys.readouterr().out


def test_refined_labels_are_fed_straight_in(ctx, capsys):
    """the output of OrganelleMembraneFilter.run_labels (device tensors) goes into the statistics without leaving the device"""
    from saber_amd.analysis import FilteringConfig, OrganelleMembraneFilter
    Z, H, W = 32, 128, 128
    org = np.zeros((Z, H, W), np.int32)
    mem = np.zeros((Z, H, W), np.uint8)
    zz, yy, xx = np.mgrid[:Z, :H, :W]
    for k, (cz, cy, cx, r) in enumerate([(16, 30, 30, 11), (15, 30, 90, 12), (17, 90, 34, 10), (16, 92, 92, 12), (14, 60, 62, 9)]):
        d2 = (zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2
        org[d2 < r * r] = k + 1
        mem[(d2 < (r + 1) ** 2) & (d2 >= (r - 2) ** 2)] = 1
    cfg = dict(ball_size=3, min_membrane_area=500, edge_trim_z=3, edge_trim_xy=3, min_roi_relative_size=0.02)
    pairs, _ = membrane_ref.refine(org, mem, **cfg)
    assert len(pairs) >= 3                                     # the scene survives refinement (CPU restatement of the pipeline)
    org_labels, _ = OrganelleMembraneFilter(FilteringConfig(**cfg)).run_labels(torch.from_numpy(org).cuda(), torch.from_numpy(mem).cuda())
    assert org_labels.is_cuda
    rows, _ = check_extract(org_labels, 10.0, capsys)
    assert len(rows) == len(pairs)


# ---------------------------------------------------------------------------------------------- scale
def torch_reference_loop(vol, labels):
    """the reference loop on the device, per label: mask == label, the count and the three coordinate sums (the moments of order 0 and 1)"""
    Z, H, W = vol.shape
    az, ay, ax = (torch.arange(s, device=vol.device, dtype=torch.int64) for s in (Z, H, W))
    out = []
    for v in labels:
        m = vol == v
        n = m.sum()
        out.append(torch.stack([n, (m.sum(dim=(1, 2)) * az).sum(), (m.sum(dim=(0, 2)) * ay).sum(), (m.sum(dim=(0, 1)) * ax).sum()]))
    return torch.stack(out)


def test_volume_scale(ctx):
    """64 x 1024 x 1024 int32 with 150 spheres (the scene of test_gpu_membranes.py::test_volume_scale): the moments equal the numpy route
    exactly; seven repetitions each of the one-pass call, its per-piece-atomics baseline and the reference loop in torch on the device.
    Asserted: the slowest one-pass repetition is below the fastest torch-loop repetition (2 reads of the volume against >= 150)."""
    rng = np.random.default_rng(9)
    Z, H, W = 64, 1024, 1024
    vol = torch.zeros((Z, H, W), dtype=torch.int32, device="cuda")
    zz = torch.arange(Z, device="cuda").view(Z, 1, 1)
    yy = torch.arange(H, device="cuda").view(1, H, 1)
    xx = torch.arange(W, device="cuda").view(1, 1, W)
    for k in range(150):
        cz, cy, cx, r = int(rng.integers(0, Z)), int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(8, 60))
        d2 = (zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2
        vol[d2 < r * r] = k + 1
    del d2
    labels, mom, stats = assert_exact(ctx, vol)
    assert labels.size >= 100
    labels_b, mom_b, _ = device_tables(ctx, vol, per_piece_atomics=True)
    assert np.array_equal(labels, labels_b) and np.array_equal(mom, mom_b)
    loop = torch_reference_loop(vol, labels.tolist()).cpu().numpy()
    assert np.array_equal(loop, mom[:, 0:4])
    torch.cuda.synchronize()
    t_one, t_base, t_loop = [], [], []
    for _ in range(7):
        t0 = time.perf_counter()
        ctx.label_statistics(vol)
        torch.cuda.synchronize()
        t_one.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ctx.label_statistics(vol, per_piece_atomics=True)
        torch.cuda.synchronize()
        t_base.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        torch_reference_loop(vol, labels.tolist())
        torch.cuda.synchronize()
        t_loop.append((time.perf_counter() - t0) * 1e3)
    gb = vol.numel() * 4 / 1e9
    line = (f"label_statistics 64x1024x1024 int32, {labels.size} labels, {int(mom[:, 0].sum())} labelled voxels, whole call (2 reads of {gb:.3f} GB): "
            f"block tables " + ", ".join(f"{t:.3f}" for t in t_one) + " ms; per-piece global atomics " + ", ".join(f"{t:.3f}" for t in t_base) +
            " ms; torch loop over the labels " + ", ".join(f"{t:.1f}" for t in t_loop) +
            f" ms; medians {np.median(t_one):.3f} / {np.median(t_base):.3f} / {np.median(t_loop):.1f} ms, torch loop / one pass = "
            f"{np.median(t_loop) / np.median(t_one):.0f}x, {2 * gb / (np.median(t_one) * 1e-3):.0f} GB/s over the whole call")
    print("\n" + line)
    TIMING_LINES["2 scale"] = line
    write_timing_file()
    assert max(t_one) < min(t_loop), "the one-pass call does not beat the per-label loop by more than the run-to-run spread"
