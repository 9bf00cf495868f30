"""Worker of tests/test_gpu_sharded_smooth.py::test_two_gloo_ranks_on_one_device: one rank of a gloo group on cuda:0 with a weight-less
engine handle runs segment_volume_sharded on device planes with sharded_stitch=True and sharded_smooth, for every gather mode, for a
volume both ranks have slices of and for a one-plane volume that leaves the second rank empty, and saves what it got - beside the
reference, which every rank computes alone: the host stitch of the whole volume, smoothed by Engine.smooth_labels."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALE = 0.05


def main(out_path):
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from saber_amd.engine import Engine
    from saber_amd.segmenters.slice_driver import segment_volume_sharded, shard_bounds
    from saber_amd.segmenters import utils
    from sharded_stitch_worker import planes_of
    eng = Engine.bare(0)
    res = {}
    for Z in (7, 1):
        vol = planes_of(Z)
        dev = torch.from_numpy(vol.view(np.int16)).cuda()
        fn = lambda z: dev[z]
        z0, z1 = shard_bounds(Z, world, rank)
        kw = dict(min_mask_area=1, engine=eng, sharded_stitch=True, sharded_smooth=SCALE)
        stitched = torch.from_numpy(utils.separate_masks(vol, min_mask_area=1).view(np.int32)).cuda()
        res[f"whole{Z}"] = eng.smooth_labels(stitched, SCALE)[0].cpu().numpy()
        t = {}
        res[f"all{Z}"] = segment_volume_sharded(vol, fn, timings=t, **kw)
        assert {"stitched", "counted", "halos", "smoothed", "gathered"} <= set(t), t
        kept = segment_volume_sharded(vol, fn, keep_on_device=True, **kw)
        assert kept.is_cuda and kept.dtype == torch.uint8
        res[f"kept{Z}"] = kept.cpu().numpy()
        r0 = segment_volume_sharded(vol, fn, gather="rank0", **kw)
        assert (r0 is None) == (rank != 0)
        if rank == 0:
            res[f"rank0{Z}"] = r0
        chunk, span = segment_volume_sharded(vol, fn, gather="none", **kw)
        assert span == (z0, z1) and tuple(chunk.shape) == (z1 - z0, 40, 48) and chunk.is_cuda and chunk.dtype == torch.uint8
        res[f"none{Z}"] = chunk.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(out_path, **res)
    dist.barrier()
    dist.destroy_process_group()
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1])
