"""Propagated label volumes: what follows the tracking loop of SAM2Adapter.segment_volume and the segmenters' merges, host route against
the opt-in device route (csrc/labelvol.hip), on one synthetic painted volume - no model.  The volume is --frames x --size^2 with
--objects balls, painted on the device from synthetic 1024^2 logits the way the adapter paints (later objects overwrite); presence
scores are a bump along z around each ball's centre, so the 0.5 threshold cuts the ends of every object.
    paint_single    the default route's painting: one saber_k_paint_nearest launch per object and frame
    paint_stack     one saber_k_paint_nearest_stack launch per frame (same volume, checked)
    host_download   vol_dev.cpu().numpy()
    host_filter     vol[f][vol[f] == obj] = 0 per frame and object below the threshold, and the .astype(np.uint16) of the return
    host_merge      np.maximum(final, (masks3d > 0).astype(np.uint8), out=final) of one seed slice
    host_stitch     utils.separate_masks (scipy, 26-connected)
    dev_filter      presence_keep_table + upload + saber_k_relabel_frames
    dev_merge       saber_k_merge_max_u16 (binarize)
    dev_stitch      Engine.separate_masks and the one download of its int32 labels
Host stages run once (they take seconds), device stages report the median of --reps after a warm-up; wall clock around a device
synchronise.  Default 128 frames; --frames 512 is the workload's size.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from saber_amd import _lib  # noqa: E402
from saber_amd.filters._context import handle  # noqa: E402
from saber_amd.segmenters import utils  # noqa: E402
from saber_amd.utils import labelvol, volprep  # noqa: E402

LOGIT_RES = 1024        # the video predictor hands logits out at its 1024^2 frame size
POOL = 8                # frames of synthetic logits kept on the device and cycled (8 x objects x 4 MB: more than the caches hold)


def balls(Z, n, seed=0):
    """centre (z, y, x) in units of the volume's extent and radius (fraction of the xy extent / of Z along z) per object"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 0.9, (n, 3)), rng.uniform(0.04, 0.12, n), rng.uniform(0.15, 0.45, n)


def frame_logits(z, Z, centres, r_xy, r_z, dev):
    """(n, LOGIT_RES, LOGIT_RES): positive inside the cross-section of each ball (an ellipsoid: r_z of the depth) on frame z"""
    g = (torch.arange(LOGIT_RES, device=dev, dtype=torch.float32) + 0.5) / LOGIT_RES
    c = torch.from_numpy(centres).to(dev, torch.float32)
    rxy, rz = torch.from_numpy(r_xy).to(dev, torch.float32), torch.from_numpy(r_z).to(dev, torch.float32)
    dz = ((z + 0.5) / Z - c[:, 0]) / rz
    d2 = ((g[None, :, None] - c[:, 1, None, None]) / rxy[:, None, None]) ** 2 + ((g[None, None, :] - c[:, 2, None, None]) / rxy[:, None, None]) ** 2
    return (1.0 - dz[:, None, None] ** 2 - d2).contiguous()


def presence(Z, centres, r_z):
    z = (np.arange(Z)[:, None] + 0.5) / Z
    return np.exp(-((z - centres[None, :, 0]) / (0.6 * r_z[None, :])) ** 2 / 2)


def timed(fn, reps=1, warm=0):
    for _ in range(warm):
        fn()
    ms = []
    out = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(f"  {statistics.median(ms):10.2f} ms", file=sys.stderr, flush=True)      # progress: the host stages of a 512-frame volume take minutes
    return out, {"median_ms": statistics.median(ms), "min_ms": min(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128, help="512 = the workload's tomogram")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true", help="device timings only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "label_volume_bench measures on the device: there is no CPU fallback"
    Z, S, n = args.frames, args.size, args.objects
    dev = torch.device("cuda:0")
    lib = _lib.load()
    eng = handle(0)
    centres, r_xy, r_z = balls(Z, n)
    ids = list(range(1, n + 1))
    res = {"frames": Z, "size": S, "objects": n, "device": torch.cuda.get_device_name(0)}

    # ---- painting: n launches per frame against one
    pool = [frame_logits(z * Z // POOL, Z, centres, r_xy, r_z, dev) for z in range(POOL)]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def paint_single(vol):
        for z in range(Z):
            lg, plane = pool[z % POOL], C.c_void_p(vol[z].data_ptr())
            for i, obj in enumerate(ids):
                if lib.saber_k_paint_nearest(C.c_void_p(lg[i].data_ptr()), LOGIT_RES, LOGIT_RES, 0.0, obj, plane, S, S, None, stream) != 0:
                    raise RuntimeError(lib.saber_k_last_error().decode())

    def paint_stack(vol):
        for z in range(Z):
            labelvol.paint_nearest_stack(pool[z % POOL], ids, vol[z])

    va = torch.zeros((Z, S, S), dtype=torch.int16, device=dev)
    vb = torch.zeros((Z, S, S), dtype=torch.int16, device=dev)
    _, res["paint_single"] = timed(lambda: paint_single(va), reps=2, warm=1)
    _, res["paint_stack"] = timed(lambda: paint_stack(vb), reps=2, warm=1)
    res["paint_same"] = bool(torch.equal(va, vb))
    res["paint_launches"] = {"single": Z * n, "stack": Z * ((n + 63) // 64)}
    del va, pool

    # ---- the volume every later stage works on: each frame from its own logits
    vb.zero_()
    for z in range(Z):
        labelvol.paint_nearest_stack(frame_logits(z, Z, centres, r_xy, r_z, dev), ids, vb[z])
    painted = vb
    res["painted_fraction"] = float((painted != 0).float().mean().item())
    bounds, thr = presence(Z, centres, r_z), 0.5
    acc0 = torch.zeros((Z, S, S), dtype=torch.int16, device=dev)
    acc0[:, : S // 16] = 1                                      # an accumulator that already holds an earlier seed's union

    # ---- device route
    def dev_filter():
        v = work.copy_(painted)
        return labelvol.relabel_frames_(v, volprep.to_device_volume(labelvol.presence_keep_table(bounds, thr), dev))

    work = torch.empty_like(painted)
    _, copy_t = timed(lambda: work.copy_(painted), reps=args.reps, warm=1)
    filtered_dev, t = timed(dev_filter, reps=args.reps, warm=1)
    res["dev_filter"] = {**t, "includes_copy_ms": copy_t["median_ms"]}      # the bench filters a copy to keep its input; the route filters in place
    acc = torch.empty_like(acc0)

    def dev_merge():
        acc.copy_(acc0)
        return labelvol.merge_max_u16_(acc, filtered_dev, binarize=True)

    merged_dev, t = timed(dev_merge, reps=args.reps, warm=1)
    res["dev_merge"] = {**t, "includes_copy_ms": copy_t["median_ms"]}

    def dev_stitch():
        labels, k = eng.separate_masks(merged_dev, 100)
        return labels.cpu().numpy().view(np.uint32), k

    (stitched_dev, k_dev), res["dev_stitch"] = timed(dev_stitch, reps=max(1, args.reps // 2), warm=1)
    res["components"] = int(k_dev)
    res["dev_total_ms"] = res["dev_filter"]["median_ms"] + res["dev_merge"]["median_ms"] + res["dev_stitch"]["median_ms"] - 2 * copy_t["median_ms"]

    # ---- host route at the parent commit's semantics
    if not args.skip_host:
        vol, res["host_download"] = timed(lambda: painted.cpu().numpy().view(np.uint16))

        def host_filter():
            for f in range(Z):
                for mi in range(n):
                    if float(bounds[f, mi]) < thr:
                        vol[f][vol[f] == mi + 1] = 0
            return vol.astype(np.uint16)

        filtered, res["host_filter"] = timed(host_filter)
        final = acc0.cpu().numpy().view(np.uint16).copy()

        def host_merge():
            masks3d = (filtered > 0).astype(np.uint8)
            np.maximum(final, masks3d, out=final)
            return final

        merged, res["host_merge"] = timed(host_merge)
        stitched, res["host_stitch"] = timed(lambda: utils.separate_masks(merged))
        res["host_total_ms"] = sum(res[k]["median_ms"] for k in ("host_download", "host_filter", "host_merge", "host_stitch"))
        res["same_filtered"] = bool(np.array_equal(filtered, filtered_dev.cpu().numpy().view(np.uint16)))
        res["same_merged"] = bool(np.array_equal(merged, merged_dev.cpu().numpy().view(np.uint16)))
        res["same_stitched"] = bool(np.array_equal(stitched, stitched_dev))
        res["host_over_device"] = res["host_total_ms"] / res["dev_total_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
