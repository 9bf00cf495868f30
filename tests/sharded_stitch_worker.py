"""Worker of tests/test_gpu_sharded_stitch.py::test_two_gloo_ranks_on_one_device: one rank of a gloo group on cuda:0 with a weight-less
engine handle runs segment_volume_sharded on device planes - the default route and sharded_stitch=True with every gather mode - for a
volume both ranks have slices of and for a one-plane volume that leaves the second rank empty, and saves what it got."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def planes_of(Z, H=40, W=48):
    rng = np.random.default_rng(100 + Z)
    vol = np.zeros((Z, H, W), dtype=np.uint16)
    zz, yy, xx = np.mgrid[:Z, :H, :W]
    for k in range(7):
        cz, cy, cx, r = rng.integers(0, Z), rng.integers(6, H - 6), rng.integers(6, W - 6), rng.integers(3, 9)
        vol[(zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k + 1
    vol[:, 2, 3] = 9
    vol[rng.random((Z, H, W)) < 0.02] = 11
    return vol


def main(out_path):
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from saber_amd.engine import Engine
    from saber_amd.segmenters.slice_driver import segment_volume_sharded, shard_bounds
    eng = Engine.bare(0)
    res = {}
    for Z in (7, 1):
        vol = planes_of(Z)
        dev = torch.from_numpy(vol.view(np.int16)).cuda()
        fn = lambda z: dev[z]
        z0, z1 = shard_bounds(Z, world, rank)
        res[f"default{Z}"] = segment_volume_sharded(vol, fn, min_mask_area=1, engine=eng)
        t = {}
        res[f"all{Z}"] = segment_volume_sharded(vol, fn, min_mask_area=1, engine=eng, sharded_stitch=True, timings=t)
        res[f"labels{Z}"] = np.array(t["labels"])
        r0 = segment_volume_sharded(vol, fn, min_mask_area=1, engine=eng, sharded_stitch=True, gather="rank0")
        assert (r0 is None) == (rank != 0)
        if rank == 0:
            res[f"rank0{Z}"] = r0
        chunk, span = segment_volume_sharded(vol, fn, min_mask_area=1, engine=eng, sharded_stitch=True, gather="none")
        assert span == (z0, z1) and tuple(chunk.shape) == (z1 - z0, 40, 48)
        if z1 > z0:
            assert isinstance(chunk, torch.Tensor) and chunk.is_cuda and chunk.dtype == torch.int32
            chunk = chunk.cpu().numpy().view(np.uint32)
        res[f"none{Z}"] = np.asarray(chunk, dtype=np.uint32)
    torch.cuda.synchronize()
    np.savez(out_path, **res)
    dist.barrier()
    dist.destroy_process_group()
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1])
