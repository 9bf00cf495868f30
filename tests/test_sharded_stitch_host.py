"""CPU: the sharded stitch (saber_amd/segmenters/stitch.py) without a device - the seam resolve on hand-made records, the host chunk
labelling composed over chunks against utils.separate_masks, and the gloo ranks of segment_volume_sharded(sharded_stitch=True) on CPU
planes for every gather mode.  Integer work: every comparison is bit for bit."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from saber_amd.segmenters import stitch, utils


def test_resolve_seams_hand_made():
    # chunk 0 holds roots 3 and 40, chunk 1 (offset 100) roots 105 and 160, chunk 2 (offset 200) root 210
    nodes = [40, 3, 105, 160, 210]
    sizes = [5, 2, 4, 1, 7]
    pairs = [[3, 105], [40, 105], [3, 105], [160, 210]]            # a U: 3 and 40 meet through 105; a repeat; a second component
    rep, total, keep = stitch.resolve_seams(nodes, sizes, pairs, 10)
    assert rep.tolist() == [3, 3, 3, 160, 160] and total.tolist() == [11, 11, 11, 8, 8] and keep.tolist() == [True] * 3 + [False] * 2
    # order of nodes and pairs does not matter
    perm = [4, 2, 0, 3, 1]
    rep2, total2, keep2 = stitch.resolve_seams([nodes[i] for i in perm], [sizes[i] for i in perm], pairs[::-1], 10)
    assert rep2.tolist() == [rep[i] for i in perm] and total2.tolist() == [total[i] for i in perm] and keep2.tolist() == [keep[i] for i in perm]
    # a node without a pair is its own component; min_voxels 0 keeps everything that has a voxel
    rep, total, keep = stitch.resolve_seams([7, 9], [1, 1], np.zeros((0, 2), np.int64), 0)
    assert rep.tolist() == [7, 9] and total.tolist() == [1, 1] and keep.all()
    rep, total, keep = stitch.resolve_seams([], [], [], 5)
    assert rep.size == 0 and total.size == 0 and keep.size == 0
    with pytest.raises(ValueError):
        stitch.resolve_seams([1, 1], [1, 1], [], 1)
    with pytest.raises(ValueError):
        stitch.resolve_seams([1, 5], [1, 1], [[1, 4]], 1)
    with pytest.raises(ValueError):
        stitch.resolve_seams([1, 5], [1], [], 1)


def test_label_chunk_host_roots_are_first_voxels():
    rng = np.random.default_rng(3)
    vol = (rng.random((4, 9, 11)) < 0.3).astype(np.uint16) * 9
    lab, sizes = stitch.label_chunk_host(vol)
    assert lab.dtype == np.uint32 and sizes.dtype == np.uint32 and lab.shape == vol.shape == sizes.shape
    assert np.array_equal(lab == stitch.NONE, vol == 0)
    flat = lab.ravel()
    roots = np.unique(flat[flat != stitch.NONE])
    for r in roots:
        member = np.flatnonzero(flat == r)
        assert member[0] == r and sizes.ravel()[r] == member.size
    assert sizes.sum() == (vol != 0).sum()
    # numbering the roots in ascending order is scipy's labelling
    ref = utils.separate_masks(vol, 0)
    assert np.array_equal(np.where(flat == stitch.NONE, 0, np.searchsorted(roots, flat) + 1).reshape(vol.shape), ref)


def _split(vol, parts):
    cuts = [round(i * vol.shape[0] / parts) for i in range(parts + 1)]
    return [vol[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def test_host_chunks_compose_to_separate_masks():
    rng = np.random.default_rng(11)
    cases = 0
    for trial in range(40):
        Z, H, W = rng.integers(1, 8), rng.integers(1, 12), rng.integers(1, 14)
        vol = (rng.random((Z, H, W)) < rng.choice([0.1, 0.3, 0.5, 0.9, 1.0])).astype(np.uint16) * rng.integers(1, 60000, (Z, H, W)).astype(np.uint16)
        for parts in (1, 2, 3, 7, 9):                               # more parts than planes: empty chunks
            for area in (0, 1, 2):
                out, n = stitch.separate_masks_chunks(None, _split(vol, parts), area)
                ref = utils.separate_masks(vol, area)
                assert np.array_equal(np.concatenate(out, 0), ref), (trial, vol.shape, parts, area)
                assert n == int(ref.max()) and all(o.dtype == np.uint32 for o in out)
                cases += 1
    assert cases == 600
    # a U: leaves chunk 0 at two places that only meet in chunk 1
    u = np.zeros((4, 5, 9), np.uint16)
    u[0:3, 2, 1] = 1
    u[0:3, 2, 7] = 2
    u[3, 2, 1:8] = 3
    for parts in (2, 4):
        out, n = stitch.separate_masks_chunks(None, _split(u, parts), 0)
        assert n == 1 and np.array_equal(np.concatenate(out, 0), utils.separate_masks(u, 0))


def test_seam_pairs_host_follows_the_merge_rule():
    N = stitch.NONE
    a = np.array([[N, 5, 5, N]], np.uint32)
    b = np.array([[7, N, N, 9]], np.uint32)
    assert stitch.seam_pairs_host(a, b).tolist() == [[5, 7], [5, 9]]
    assert stitch.seam_pairs_host(a, b, 100, 200).tolist() == [[105, 207], [105, 209]]
    b = np.array([[7, 8, N, 9]], np.uint32)                         # centre foreground: its diagonals are not looked at
    assert stitch.seam_pairs_host(np.array([[N, 5, N, N]], np.uint32), b).tolist() == [[5, 8]]
    assert stitch.seam_pairs_host(np.full((2, 3), N, np.uint32), np.zeros((2, 3), np.uint32)).shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------- gloo ranks, CPU planes
def _planes(Z, H, W):
    rng = np.random.default_rng(Z)
    vol = np.zeros((Z, H, W), dtype=np.uint16)
    zz, yy, xx = np.mgrid[:Z, :H, :W]
    for k in range(7):
        cz, cy, cx, r = rng.integers(0, Z), rng.integers(6, H - 6), rng.integers(6, W - 6), rng.integers(3, 9)
        vol[(zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k + 1
    vol[:, 2, 3] = 9                                                # a column through every chunk
    vol[rng.random((Z, H, W)) < 0.02] = 11                          # specks: small components on and off the seams
    return vol


def _worker(rank, world, port, Z, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from saber_amd.segmenters.slice_driver import segment_volume_sharded, shard_bounds
        vol = _planes(Z, 40, 48)
        slice_fn = lambda z: torch.from_numpy(vol[z].astype(np.int16))
        z0, z1 = shard_bounds(Z, world, rank)
        res = {"default": segment_volume_sharded(vol, slice_fn, min_mask_area=1)}
        for area in (0, 1):
            t = {}
            res[f"all{area}"] = segment_volume_sharded(vol, slice_fn, min_mask_area=area, sharded_stitch=True, gather="all", timings=t)
            assert {"segmented", "labelled", "resolved", "stitched", "gathered", "labels"} <= set(t), t
            res[f"labels{area}"] = np.array(t["labels"])
            r0 = segment_volume_sharded(vol, slice_fn, min_mask_area=area, sharded_stitch=True, gather="rank0")
            assert (r0 is None) == (rank != 0)
            if rank == 0:
                res[f"rank0{area}"] = r0
            chunk, span = segment_volume_sharded(vol, slice_fn, min_mask_area=area, sharded_stitch=True, gather="none")
            assert span == (z0, z1) and isinstance(chunk, np.ndarray) and chunk.dtype == np.uint32 and chunk.shape == (z1 - z0, 40, 48)
            res[f"none{area}"] = chunk
        with pytest.raises(ValueError):
            segment_volume_sharded(vol, slice_fn, sharded_stitch=True, smooth_scale=0.05)
        with pytest.raises(ValueError):
            segment_volume_sharded(vol, slice_fn, sharded_stitch=True, gather="some")
        np.savez(os.path.join(out_dir, f"out{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,Z", [(2, 7), (2, 8), (3, 7), (3, 8), (3, 2)])
def test_sharded_stitch_gloo_cpu_planes(tmp_path, world, Z):
    from saber_amd.segmenters.slice_driver import shard_bounds
    port = 31500 + (os.getpid() % 2000) + 10 * world + Z
    mp.spawn(_worker, args=(world, port, Z, str(tmp_path)), nprocs=world, join=True)
    vol = _planes(Z, 40, 48)
    got = [np.load(tmp_path / f"out{r}.npz") for r in range(world)]
    assert np.array_equal(got[0]["default"], utils.separate_masks(vol, min_mask_area=1))
    for area in (0, 1):
        ref = utils.separate_masks(vol, min_mask_area=area)
        assert ref.max() > 1
        for r in range(world):
            a, b = shard_bounds(Z, world, r)
            assert got[r][f"all{area}"].dtype == np.uint32 and np.array_equal(got[r][f"all{area}"], ref), (area, r)
            assert np.array_equal(got[r][f"none{area}"], ref[a:b]), (area, r)
            assert int(got[r][f"labels{area}"]) == int(ref.max())
        assert np.array_equal(got[0][f"rank0{area}"], ref)
    assert np.array_equal(got[0]["all1"], got[0]["default"])


def test_sharded_stitch_single_process_host_route():
    from saber_amd.segmenters.slice_driver import segment_volume_sharded
    vol = _planes(5, 40, 48)
    slice_fn = lambda z: torch.from_numpy(vol[z].astype(np.int16))
    ref = utils.separate_masks(vol, min_mask_area=1)
    assert np.array_equal(segment_volume_sharded(vol, slice_fn, min_mask_area=1, sharded_stitch=True), ref)
    chunk, span = segment_volume_sharded(vol, slice_fn, min_mask_area=1, sharded_stitch=True, gather="none")
    assert span == (0, 5) and np.array_equal(chunk, ref)
