"""The stitch over z-chunks (saber_amd/segmenters/stitch.py, csrc/cc3d.hip) against the whole-volume stitch, one process on one device,
on a --frames x --size^2 volume of blobs (no model).  The ranks of world 2, 4 and 8 are simulated one after the other: what one rank
would run is timed per chunk and the slowest chunk is reported.
    whole            Engine.separate_masks on the whole volume (what every rank runs without sharded_stitch)
    label            Engine.cc_chunk_label of a chunk
    seam             Engine.cc_seam_pairs of a seam (kernel, download of the pairs, np.unique)
    faces            the unique roots of the facing planes and their sizes (torch.unique on one or two planes, download)
    resolve          resolve_seams over every rank's record + the id table (host, identical on every rank)
    roots            Engine.cc_chunk_roots (kept non-seam roots; sorted on the host)
    finish           Engine.cc_chunk_finish (assign + relabel)
Device stages by device events around the call (they include the call's own transfers), `resolve` by the host clock; the median of --reps
after a warm-up.  Also: the bytes a rank sends and receives per gather mode beside the plane all-gather of the default route, and the
device memory a rank needs.  The chunks' labels are compared with the whole-volume result.  Multi-GPU wall clock is not measured here:
one device.  Prints one JSON line."""
import argparse
import json
import os
import pickle
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from saber_amd.engine import Engine  # noqa: E402
from saber_amd.segmenters import stitch  # noqa: E402
from saber_amd.segmenters.slice_driver import shard_bounds  # noqa: E402


def blob_volume(Z, S, dev, seed=0):
    """int16 planes with 40 large and 400 small balls, values 1..440 (later balls overwrite)"""
    rng = np.random.default_rng(seed)
    vol = torch.zeros((Z, S, S), dtype=torch.int16, device=dev)
    radii = np.concatenate([rng.uniform(0.03, 0.10, 40), rng.uniform(0.003, 0.012, 400)]) * S
    for k, r in enumerate(radii):
        c = rng.uniform(0, 1, 3) * (Z, S, S)
        lo = np.maximum(np.floor(c - r).astype(int), 0)
        hi = np.minimum(np.ceil(c + r).astype(int) + 1, (Z, S, S))
        if np.any(hi <= lo):
            continue
        g = [torch.arange(lo[i], hi[i], device=dev, dtype=torch.float32) - float(c[i]) for i in range(3)]
        inside = g[0][:, None, None] ** 2 + g[1][None, :, None] ** 2 + g[2][None, None, :] ** 2 < r * r
        vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].masked_fill_(inside, k + 1)
    return vol


def dev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def one_world(eng, vol, world, min_mask_area):
    """one pass over the ranks of `world`; returns (per-stage ms: the slowest rank's, record bytes, labels, n)"""
    Z, H, W = vol.shape
    ops = stitch._DeviceOps(eng)
    bounds = [shard_bounds(Z, world, r) for r in range(world)]
    ms = {k: 0.0 for k in ("label", "seam", "faces", "resolve", "roots", "finish")}
    chunks = []
    for a, b in bounds:
        c, t = dev_ms(lambda: stitch._Chunk(ops, vol[a:b], a, H, W))
        chunks.append(c)
        ms["label"] = max(ms["label"], t)
    records = []
    for r, c in enumerate(chunks):
        faces = sorted(set(([0] if r > 0 else []) + ([c.Zc - 1] if r + 1 < world else [])))
        sz, pairs = stitch._E, stitch._E.reshape(0, 2)
        if faces:
            (c.seam_local, sz), t = dev_ms(lambda: ops.face_nodes(c.lab, c.sizes, faces))
            ms["faces"] = max(ms["faces"], t)
        if r + 1 < world:
            n = chunks[r + 1]
            pairs, t = dev_ms(lambda: ops.seam_pairs(ops.plane(c.lab, c.Zc - 1), c.off, n.first_plane(), n.off))
            ms["seam"] = max(ms["seam"], t)
        records.append((c.seam_local + c.off, sz, pairs))
    min_voxels = stitch.min_voxels_of(min_mask_area)
    t0 = time.perf_counter()
    resolved = stitch._resolve_records(records, min_voxels)
    ms["resolve"] = (time.perf_counter() - t0) * 1e3
    owns = []
    for c in chunks:
        o, t = dev_ms(lambda: c.own(resolved, min_voxels))
        owns.append(o)
        ms["roots"] = max(ms["roots"], t)
    t0 = time.perf_counter()
    prefix, table, total = stitch._id_table(owns)
    ms["resolve"] += (time.perf_counter() - t0) * 1e3
    labels = []
    for r, c in enumerate(chunks):
        lab, t = dev_ms(lambda: c.finish(resolved, table, int(prefix[r])))
        labels.append(lab)
        ms["finish"] = max(ms["finish"], t)
    rec_bytes = sum(len(pickle.dumps(x)) for x in records) + sum(len(pickle.dumps(x)) for x in owns)
    return ms, rec_bytes, labels, total, sum(len(x[2]) for x in records), sum(len(x[0]) for x in records)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512, help="512 = the workload's tomogram")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--worlds", default="2,4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-mask-area", type=int, default=100)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = Engine.bare(0)
    Z, S = args.frames, args.size
    vol = blob_volume(Z, S, dev)
    n_vox = Z * S * S
    res = {"what": "stitch over z-chunks against the whole-volume stitch, one device, ranks simulated in sequence",
           "volume": [Z, S, S], "min_mask_area": args.min_mask_area, "foreground_fraction": float((vol != 0).float().mean().item())}
    eng.separate_masks(vol, args.min_mask_area)                     # warm-up
    t = []
    for _ in range(args.reps):
        (whole, n_whole), m = dev_ms(lambda: eng.separate_masks(vol, args.min_mask_area))
        t.append(m)
    res["whole"] = {"median_ms": statistics.median(t), "min_ms": min(t), "labels": n_whole,
                    "workspace_bytes": n_vox * 8, "gathered_plane_bytes": n_vox * 2}
    plane = S * S * 4
    for world in [int(w) for w in args.worlds.split(",")]:
        one_world(eng, vol, world, args.min_mask_area)              # warm-up
        runs = [one_world(eng, vol, world, args.min_mask_area) for _ in range(args.reps)]
        ms = {k: statistics.median(r[0][k] for r in runs) for k in runs[0][0]}
        _, rec_bytes, labels, total, n_pairs, n_nodes = runs[-1]
        same = torch.equal(torch.cat(labels, 0), whole) and total == n_whole
        chunk = max(b - a for a, b in (shard_bounds(Z, world, r) for r in range(world)))
        res[f"world{world}"] = {
            "ms": ms, "rank_total_ms": sum(ms.values()), "equal_to_whole": bool(same), "labels": total, "seam_nodes": n_nodes, "seam_pairs": n_pairs,
            "bytes_per_rank": {
                "default_route_plane_all_gather_recv": world * chunk * S * S * 2,
                "first_planes_sent": plane, "first_planes_recv": world * plane, "records_recv": rec_bytes,
                "labels_gather_all_recv": world * chunk * plane, "labels_gather_rank0_sent": chunk * plane, "labels_gather_none": 0},
            "workspace_bytes_per_rank": chunk * S * S * 8 + S * S * 8 + world * plane,
        }
        del labels, runs
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
