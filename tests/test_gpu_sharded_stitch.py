"""GPU: the stitch over z-chunks (csrc/cc3d.hip: saber_cc_chunk_label / saber_cc_seam_pairs / saber_cc_chunk_roots / saber_cc_chunk_finish;
saber_amd/segmenters/stitch.py) against utils.separate_masks and Engine.separate_masks on the whole volume.  Integer work: every
comparison is bit for bit.  The splits are 1, 2, 3 and Z chunks (Z chunks = one plane each: every plane faces both neighbours)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from saber_amd.segmenters import stitch, utils

pytestmark = pytest.mark.gpu
NONE = stitch.NONE


def _split(vol, parts):
    cuts = [round(i * vol.shape[0] / parts) for i in range(parts + 1)]
    return [vol[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def check(engine, vol, areas=(0, 1, 2), splits=None):
    """separate_masks_chunks of `vol` for every split and area against the host and the whole-volume device stitch"""
    vol = np.ascontiguousarray(vol, dtype=np.uint16)
    dev = torch.from_numpy(vol.view(np.int16)).cuda()
    Z = vol.shape[0]
    for area in areas:
        ref = utils.separate_masks(vol, min_mask_area=area)
        whole, n_whole = engine.separate_masks(dev, min_mask_area=area)
        assert np.array_equal(whole.cpu().numpy().view(np.uint32), ref)
        for parts in sorted(set(splits or (1, 2, 3, Z))):
            chunks = [c.contiguous() for c in _split(dev, parts)]
            out, n = stitch.separate_masks_chunks(engine, chunks, area)
            assert all(o.dtype == torch.int32 and o.is_cuda and o.shape == c.shape for o, c in zip(out, chunks))
            got = torch.cat(out, 0).cpu().numpy().view(np.uint32)
            assert np.array_equal(got, ref), (vol.shape, area, parts)
            assert n == n_whole == int(ref.max())
    return ref


@pytest.mark.parametrize("shape", [(6, 17, 67), (7, 9, 130)])
@pytest.mark.parametrize("density", [0.1, 0.3, 0.5, 0.9])
def test_speckle(engine, shape, density):
    rng = np.random.default_rng(int(density * 10) + shape[0])
    vol = (rng.random(shape) < density).astype(np.uint16) * rng.integers(1, 60000, shape).astype(np.uint16)
    check(engine, vol)


def test_blobs(engine):
    rng = np.random.default_rng(4)
    Z, H, W = 12, 40, 70
    vol = np.zeros((Z, H, W), np.uint16)
    zz, yy, xx = np.mgrid[:Z, :H, :W]
    for k in range(14):
        cz, cy, cx, r = rng.integers(0, Z), rng.integers(0, H), rng.integers(0, W), rng.integers(2, 8)
        vol[(zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k + 1
    ref = check(engine, vol)
    assert ref.max() >= 1


def test_full_and_empty(engine):
    check(engine, np.ones((5, 7, 66), np.uint16))
    ref = check(engine, np.zeros((4, 6, 65), np.uint16))
    assert ref.max() == 0


def test_u_shape_joins_two_roots_of_chunk_0(engine):
    """two columns start in chunk 0, run down through the seam and only meet in the last plane: chunk 0 holds two roots of one component"""
    u = np.zeros((6, 5, 70), np.uint16)
    u[0:5, 2, 1] = 1
    u[0:5, 2, 66] = 2
    u[5, 2, 1:67] = 3
    u[0, 4, 30] = 4                                                 # a second component between the two roots in scan order
    ref = check(engine, u, areas=(0,))
    assert ref.max() == 2 and ref[0, 2, 66] == 1 and ref[0, 4, 30] == 2


def test_column_through_one_plane_chunks(engine):
    v = np.zeros((9, 4, 65), np.uint16)
    v[:, 1, 64] = 5
    v[3, 3, 0] = 1                                                  # and a voxel of its own in the middle
    ref = check(engine, v, areas=(0,), splits=(9, 4))
    assert ref.max() == 2 and ref[0, 1, 64] == 1 and ref[8, 1, 64] == 1
    assert check(engine, v, areas=(1,), splits=(9,)).max() == 0      # 9 voxels, one per chunk: below 10 together as well


def test_diagonal_contact_only(engine):
    d = np.zeros((2, 4, 130), np.uint16)
    d[0, 1, 5] = 1
    d[1, 2, 6] = 1                                                  # (z+1, y+1, x+1)
    d[0, 2, 63] = 2
    d[1, 1, 64] = 2                                                 # across the wave boundary x = 63 | 64, (z+1, y-1, x+1)
    d[0, 0, 100] = 3
    d[1, 0, 102] = 3                                                # two apart: no contact
    ref = check(engine, d, areas=(0,), splits=(1, 2))
    assert ref.max() == 4
    e = np.zeros((2, 3, 128), np.uint16)
    e[0, 1, 64] = 1
    e[1, 1, 63] = 1                                                 # (z+1, y, x-1) across 63 | 64
    assert check(engine, e, areas=(0,), splits=(2,)).max() == 1


def test_pieces_reach_min_vol_only_together(engine):
    """min_mask_area 1 = 10 voxels: a bar of 6 + 6 voxels across the seam is kept, one of 4 + 4 is dropped, a bar of 12 inside a chunk is kept"""
    v = np.zeros((4, 6, 70), np.uint16)
    v[1, 1, 2:8] = 1
    v[2, 1, 2:8] = 1
    v[1, 3, 60:64] = 2
    v[2, 3, 62:66] = 2
    v[0, 5, 10:22] = 3
    v[3, 5, 10:19] = 4                                              # 9 voxels inside a chunk: dropped
    ref = check(engine, v, areas=(1,), splits=(2, 4))
    assert ref.max() == 2 and ref[1, 1, 2] == 2 and ref[2, 1, 7] == 2 and ref[1, 3, 60] == 0 and ref[0, 5, 10] == 1 and ref[3, 5, 10] == 0


def test_touching_planes_with_different_label_values(engine):
    v = np.zeros((4, 8, 66), np.uint16)
    v[0:2, 2:6, 10:60] = 7
    v[2:4, 3:7, 20:66] = 65535                                      # a different label value on the other side of the seam: one component
    assert check(engine, v, splits=(2, 4)).max() == 1


def test_first_voxel_two_chunks_before_the_bulk(engine):
    v = np.zeros((6, 8, 66), np.uint16)
    v[0, 0, 65] = 1                                                 # a thread from the first plane ...
    v[1, 1, 64] = 1
    v[2, 2, 63] = 1
    v[3, 3, 62] = 1
    v[4:6, 2:8, 0:64] = 2                                           # ... to a block two chunks later
    v[0, 5, 5] = 3                                                  # comes after the thread's first voxel, before the block
    ref = check(engine, v, areas=(0, 1), splits=(3, 6))
    assert ref[5, 7, 0] == 1


# ---------------------------------------------------------------------------------------------------------------- the seam kernel alone
def seam_pairs_loops(a, b):
    """the pairs of cc_seam_pairs by a double loop over the pixels: per row offset the centre if it is foreground, else the diagonals"""
    H, W = a.shape
    out = set()
    for y in range(H):
        for x in range(W):
            if a[y, x] == NONE:
                continue
            for dy in (-1, 0, 1):
                yy = y + dy
                if yy < 0 or yy >= H:
                    continue
                if b[yy, x] != NONE:
                    out.add((int(a[y, x]), int(b[yy, x])))
                    continue
                for xx in (x - 1, x + 1):
                    if 0 <= xx < W and b[yy, xx] != NONE:
                        out.add((int(a[y, x]), int(b[yy, xx])))
    return np.array(sorted(out), dtype=np.int64).reshape(-1, 2)


@pytest.mark.parametrize("shape", [(1, 1), (3, 70), (17, 129)])
def test_seam_pairs_against_loops(engine, shape):
    rng = np.random.default_rng(shape[1])
    for da, db, runs in ((0.5, 0.5, False), (0.9, 0.2, False), (1.0, 1.0, False), (0.6, 0.6, True), (0.0, 0.7, False)):
        a = np.where(rng.random(shape) < da, rng.integers(0, 40, shape), NONE).astype(np.uint32)
        b = np.where(rng.random(shape) < db, rng.integers(0, 40, shape), NONE).astype(np.uint32)
        if runs:                                                    # x-neighbours share their root, as the planes of a labelling do
            a, b = stitch.label_chunk_host(a[None] != NONE)[0][0], stitch.label_chunk_host(b[None] != NONE)[0][0]
        ad, bd = torch.from_numpy(a.view(np.int32)).cuda(), torch.from_numpy(b.view(np.int32)).cuda()
        ref = seam_pairs_loops(a, b)
        got = engine.cc_seam_pairs(ad, bd)
        assert got.dtype == np.int64 and np.array_equal(got, ref), (shape, da, db)
        assert np.array_equal(engine.cc_seam_pairs(ad, bd), got)                       # a second call: the same array
        assert np.array_equal(engine.cc_seam_pairs(ad, bd, capacity=1), got)           # overflow reported, retried with room for all
        assert np.array_equal(stitch.seam_pairs_host(a, b), ref)
        assert np.array_equal(engine.cc_seam_pairs(ad, bd, 1000, 5000), ref + np.array([1000, 5000]) if ref.size else ref)


def test_error_paths(engine):
    lib, h = engine.lib, engine.h
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = C.c_int(-7)
    planes = torch.ones((2, 3, 5), dtype=torch.int16).cuda()
    lab, sizes = engine.cc_chunk_label(planes)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.saber_cc_chunk_label(h, None, 2, 3, 5, p(lab), p(sizes), st) == -1 and b"cc_chunk_label:" in lib.saber_last_error(h)
    assert lib.saber_cc_chunk_label(h, p(planes), 0, 3, 5, p(lab), p(sizes), st) == -1 and b"cc_chunk_label:" in lib.saber_last_error(h)
    assert lib.saber_cc_chunk_label(h, p(planes), 1 << 11, 1 << 10, 1 << 10, p(lab), p(sizes), st) == -1 and b"2^31" in lib.saber_last_error(h)
    assert lib.saber_cc_seam_pairs(h, p(lab), None, 3, 5, 0, 0, None, 0, C.byref(n), st) == -1 and b"cc_seam_pairs:" in lib.saber_last_error(h)
    assert lib.saber_cc_seam_pairs(h, p(lab), p(lab), 3, 5, 0, 0, None, 4, C.byref(n), st) == -1 and b"cc_seam_pairs:" in lib.saber_last_error(h)
    assert lib.saber_cc_chunk_roots(h, p(lab), None, 2, 3, 5, 1, None, 0, None, 0, C.byref(n), st) == -1 and b"cc_chunk_roots:" in lib.saber_last_error(h)
    assert lib.saber_cc_chunk_finish(h, None, p(sizes), 2, 3, 5, None, None, 0, st) == -1 and b"cc_chunk_finish:" in lib.saber_last_error(h)
    # a capacity that is too small: the count is reported, nothing past the buffer is written
    a = torch.zeros((3, 5), dtype=torch.int32).cuda()
    a[:, 1] = 4
    b = torch.full((3, 5), 9, dtype=torch.int32).cuda()
    buf = torch.full((4, 2), -5, dtype=torch.int32).cuda()
    assert lib.saber_cc_seam_pairs(h, p(a), p(b), 3, 5, 0, 0, p(buf), 2, C.byref(n), st) == -4 and b"cc_seam_pairs:" in lib.saber_last_error(h)
    assert n.value > 2 and (buf[2:] == -5).all() and (buf[:2] != -5).all()
    full = n.value
    buf = torch.empty((full, 2), dtype=torch.int32).cuda()
    assert lib.saber_cc_seam_pairs(h, p(a), p(b), 3, 5, 0, 0, p(buf), full, C.byref(n), st) == 0 and n.value == full
    out = np.empty(1, np.uint32)
    two = torch.zeros((1, 3, 5), dtype=torch.int16).cuda()
    two[0, 0, 0] = two[0, 2, 0] = two[0, 2, 4] = 1
    l2, s2 = engine.cc_chunk_label(two)
    assert lib.saber_cc_chunk_roots(h, p(l2), p(s2), 1, 3, 5, 1, None, 0, out.ctypes.data_as(C.c_void_p), 1, C.byref(n), st) == -4 and n.value == 3
    assert engine.cc_chunk_roots(l2, s2, 1).tolist() == [0, 10, 14] and engine.cc_chunk_roots(l2, s2, 1, exclude=[10]).tolist() == [0, 14]
    # the wrapper's own checks: shapes, dtypes, roots outside the chunk
    with pytest.raises(ValueError):
        engine.cc_chunk_label(planes.to(torch.int32))
    with pytest.raises(ValueError):
        engine.cc_chunk_label(planes.cpu())
    with pytest.raises(ValueError):
        engine.cc_seam_pairs(lab[0], lab[:, :2][0].contiguous())
    with pytest.raises(ValueError):
        engine.cc_chunk_roots(lab, sizes[:1], 1)
    with pytest.raises(ValueError, match="outside the chunk"):
        engine.cc_chunk_roots(lab, sizes, 1, exclude=[30])
    with pytest.raises(ValueError, match="outside the chunk"):
        engine.cc_chunk_finish(lab, sizes, [30], [1])
    with pytest.raises(ValueError):
        engine.cc_chunk_finish(lab, sizes, [0, 1], [1])
    with pytest.raises(ValueError):
        stitch.separate_masks_chunks(engine, [planes, planes[:, :2].contiguous()])


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_driver_single_process_device_route(engine):
    from saber_amd.segmenters.slice_driver import segment_volume_sharded
    from sharded_stitch_worker import planes_of
    vol = planes_of(5)
    dev = torch.from_numpy(vol.view(np.int16)).cuda()
    ref = utils.separate_masks(vol, min_mask_area=1)
    t = {}
    out = segment_volume_sharded(vol, lambda z: dev[z], min_mask_area=1, engine=engine, sharded_stitch=True, timings=t)
    assert out.dtype == np.uint32 and np.array_equal(out, ref) and t["labels"] == int(ref.max()) and {"labelled", "resolved", "stitched"} <= set(t)
    kept = segment_volume_sharded(vol, lambda z: dev[z], min_mask_area=1, engine=engine, sharded_stitch=True, keep_on_device=True)
    assert kept.is_cuda and kept.dtype == torch.int32 and np.array_equal(kept.cpu().numpy().view(np.uint32), ref)
    with pytest.raises(ValueError):
        segment_volume_sharded(vol, lambda z: dev[z], engine=engine, sharded_stitch=True, smooth_scale=0.05)


def test_two_gloo_ranks_on_one_device(tmp_path):
    """two gloo ranks on this one GPU (RCCL needs a GPU per rank) with weight-less handles: device planes, collectives staged through the
    host; Z = 7 (chunks of 4 + 3 planes) and Z = 1 (the second rank owns nothing)"""
    from saber_amd.segmenters.slice_driver import shard_bounds
    from sharded_stitch_worker import planes_of
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sharded_stitch_worker.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    procs = []
    for r in range(2):                                              # the ranks meet at the rendezvous: both have to be running
        e = dict(env, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29700 + os.getpid() % 200))
        procs.append(subprocess.Popen([sys.executable, worker, str(tmp_path / f"r{r}.npz")], env=e))
    status = []
    try:
        for p_ in procs:
            status.append(p_.wait(timeout=180))
    finally:
        for p_ in procs:
            if p_.poll() is None:
                p_.kill()
                p_.wait()
    assert status == [0, 0], status
    got = [np.load(str(tmp_path / f"r{r}.npz")) for r in range(2)]
    for Z in (7, 1):
        ref = utils.separate_masks(planes_of(Z), min_mask_area=1)
        assert ref.max() >= 1
        for r in range(2):
            a, b = shard_bounds(Z, 2, r)
            assert np.array_equal(got[r][f"default{Z}"], ref) and np.array_equal(got[r][f"all{Z}"], ref), (Z, r)
            assert np.array_equal(got[r][f"none{Z}"], ref[a:b]) and int(got[r][f"labels{Z}"]) == int(ref.max()), (Z, r)
        assert np.array_equal(got[0][f"rank0{Z}"], ref)


def test_sharded_stitch_over_rccl_world_size_one(engine):
    """the NCCL (= RCCL) form on the one GPU: world size 1 through the driver, and the collectives the N > 1 branch issues (the byte-view
    all-gather of an int32 plane, all_gather_object of a record)"""
    import torch.distributed as dist
    from saber_amd.segmenters.slice_driver import segment_volume_sharded
    from sharded_stitch_worker import planes_of
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29900 + os.getpid() % 90))
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        assert dist.get_backend() == "nccl"
        vol = planes_of(5)
        dev = torch.from_numpy(vol.view(np.int16)).cuda()
        ref = utils.separate_masks(vol, min_mask_area=1)
        for mode in ("all", "rank0"):
            out = segment_volume_sharded(vol, lambda z: dev[z], min_mask_area=1, engine=engine, sharded_stitch=True, gather=mode)
            assert np.array_equal(out, ref)
        chunk, span = segment_volume_sharded(vol, lambda z: dev[z], min_mask_area=1, engine=engine, sharded_stitch=True, gather="none")
        assert span == (0, 5) and chunk.is_cuda and np.array_equal(chunk.cpu().numpy().view(np.uint32), ref)
        lab, _ = engine.cc_chunk_label(dev)
        firsts = torch.empty((1,) + tuple(lab[0].shape), dtype=torch.int32, device=lab.device)
        stitch._all_gather_bytes(dist, firsts, lab[0], None)
        torch.cuda.synchronize()
        assert torch.equal(firsts[0], lab[0])
        record = (np.arange(3), np.arange(3) + 1, np.zeros((0, 2), np.int64))
        got = [None]
        dist.all_gather_object(got, record)
        assert all(np.array_equal(x, y) for x, y in zip(got[0], record))
    finally:
        if created:
            dist.destroy_process_group()
