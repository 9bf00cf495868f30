"""The smoothing over z-chunks (saber_amd/segmenters/smooth.py, csrc/smooth3d.hip: saber_smooth_labels_chunk) against Engine.smooth_labels on
the whole volume, one process on one device, on the stitched labels of the --frames x --size^2 ball volume of tools/sharded_stitch_bench.py
(no model).  The ranks of world 2, 4 and 8 are simulated one after the other: what one rank would run is timed per chunk and the slowest
chunk is reported per stage.
    whole            Engine.smooth_labels on the whole volume (what one rank runs after gathering the labels)
    count            Engine.label_max + Engine.label_counts of the own planes (the tables are then summed: a world-sized all-reduce)
    halo             the copy of the halo planes into buffers of their own (what arrives from the neighbours; the transfer itself is not here)
    chunk            the one Engine.smooth_labels_chunk call
Host clock around each call behind a device synchronisation (the calls synchronise themselves and include their host work); the median of
--reps after a warm-up.  Also per world: halo depth, bytes a rank receives before its chunk call, the device memory the chunk call takes
(free device memory sampled from a second thread while the call runs) and the bytes a rank hands to the gather beside the 4 B/voxel of the
label gather.  Every world's concatenated chunks are compared with `whole`: the run fails if they differ.  Multi-GPU wall clock is not
measured here: one device.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from saber_amd.engine import Engine  # noqa: E402
from saber_amd.segmenters import smooth  # noqa: E402
from saber_amd.segmenters.slice_driver import shard_bounds  # noqa: E402
from sharded_stitch_bench import blob_volume  # noqa: E402


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def peak_bytes(fn):
    """device memory `fn` takes at its peak: the smallest free memory a second thread sees while it runs, against the free memory before"""
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    low, stop = [before], threading.Event()

    def watch():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
    th = threading.Thread(target=watch)
    th.start()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        stop.set()
        th.join()
    return int(before - low[0])


def one_world(eng, labels, world, scale):
    """one pass over the ranks of `world`; returns (per-stage ms of the slowest rank, halo depth, most bytes received, the chunks)"""
    Z, H, W = labels.shape
    bounds = [shard_bounds(Z, world, r) for r in range(world)]
    ms = {"count": 0.0, "halo": 0.0, "chunk": 0.0}
    tables, m = [], 0
    for a, b in bounds:
        c = labels[a:b]
        mx, t1 = host_ms(lambda: eng.label_max(c))
        m = max(m, mx)
        tables.append((c, t1))
    counts = None
    for c, t1 in tables:
        tab, t2 = host_ms(lambda: eng.label_counts(c, m + 1))
        counts = tab if counts is None else counts + tab
        ms["count"] = max(ms["count"], t1 + t2)
    ids, cnt, h = smooth._table(eng, counts.cpu().numpy(), scale)
    out, recv = [], 0
    for r, (a, b) in enumerate(bounds):
        plan = smooth.halo_plan(bounds, r, h)
        pieces = {side: [labels[p:q] for _, p, q in plan[side]] for side in ("lo", "hi")}
        (lo, hi), t = host_ms(lambda: tuple(torch.cat(pieces[s], 0) if pieces[s] else None for s in ("lo", "hi")))
        ms["halo"] = max(ms["halo"], t)
        n_lo, n_hi = (0 if x is None else int(x.shape[0]) for x in (lo, hi))
        recv = max(recv, (n_lo + n_hi) * H * W * labels.element_size() + 8 * (m + 1))
        (o, _), t = host_ms(lambda: eng.smooth_labels_chunk(labels[a:b], lo, hi, ids, cnt, scale, a - n_lo == 0, b + n_hi == Z))
        ms["chunk"] = max(ms["chunk"], t)
        out.append(o)
    return ms, h, recv, out, (ids, cnt, bounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512, help="512 = the workload's tomogram")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--worlds", default="2,4,8")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=0.05, help="segment_tomogram_core's")
    ap.add_argument("--min-mask-area", type=int, default=100)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = Engine.bare(0)
    Z, S = args.frames, args.size
    labels, n_labels = eng.separate_masks(blob_volume(Z, S, dev), args.min_mask_area)
    n_vox = Z * S * S
    res = {"what": "smoothing over z-chunks against the whole-volume smoothing, one device, ranks simulated in sequence",
           "volume": [Z, S, S], "scale": args.scale, "labels": n_labels, "foreground_fraction": float((labels != 0).float().mean().item())}
    eng.smooth_labels(labels, args.scale)                           # warm-up
    t = []
    for _ in range(args.reps):
        (whole, _), m = host_ms(lambda: eng.smooth_labels(labels, args.scale))
        t.append(m)
    res["whole"] = {"median_ms": statistics.median(t), "min_ms": min(t), "gathered_label_bytes": n_vox * 4,
                    "workspace_peak_bytes": peak_bytes(lambda: eng.smooth_labels(labels, args.scale))}
    for world in [int(w) for w in args.worlds.split(",")]:
        one_world(eng, labels, world, args.scale)                   # warm-up
        runs = [one_world(eng, labels, world, args.scale) for _ in range(args.reps)]
        ms = {k: statistics.median(r[0][k] for r in runs) for k in runs[0][0]}
        _, h, recv, out, (ids, cnt, bounds) = runs[-1]
        same = torch.equal(torch.cat(out, 0), whole)
        del out, runs
        r_mid = world // 2                                          # a rank with two neighbours
        a, b = bounds[r_mid]
        plan = smooth.halo_plan(bounds, r_mid, h)
        lo, hi = (torch.cat([labels[p:q] for _, p, q in plan[s]], 0) if plan[s] else None for s in ("lo", "hi"))
        n_lo, n_hi = (0 if x is None else int(x.shape[0]) for x in (lo, hi))
        peak = peak_bytes(lambda: eng.smooth_labels_chunk(labels[a:b], lo, hi, ids, cnt, args.scale, a - n_lo == 0, b + n_hi == Z))
        depth = max(q - p for p, q in bounds)
        res[f"world{world}"] = {
            "ms": ms, "rank_total_ms": sum(ms.values()), "equal_to_whole": bool(same), "halo_depth": h, "chunk_planes": depth,
            "bytes_received_before_chunk_call": recv,
            "workspace_peak_bytes_chunk_call": peak, "winner_bytes": depth * S * S * 4, "halo_buffer_bytes": (n_lo + n_hi) * S * S * 4,
            "bytes_to_gather_uint8": depth * S * S, "bytes_to_gather_labels": depth * S * S * 4,
        }
        assert same, f"world {world}: the chunks differ from the whole-volume result"
    last = res[f"world{args.worlds.split(',')[-1]}"]
    res["last_world_rank_total_below_whole"] = bool(last["rank_total_ms"] < res["whole"]["median_ms"])
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
