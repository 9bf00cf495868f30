"""Consensus mask resolution of the classifier filter (saber_amd/filters/masks.py: _consensus_based_resolution), host route against the
opt-in device route (csrc/consensus2d.hip), on the same disc masks:
    host          the unchanged numpy / scipy.ndimage.label code, dict list in, dict list out
    box_upload    the device route, dict list in, dict list out: builds and uploads the uint8 stack, Engine.consensus_components,
                  downloads the label plane, builds every component's full-size bool array
    box_resident  the same with the stack already on the device (masks_dev=, what apply_classifier(device=) does: its upload is shared
                  with the classifier)
    engine        Engine.consensus_components alone on the resident stack: kernels, one synchronisation, the table's download
Wall clock (time.perf_counter) after a warm-up call, median and minimum over --reps (host: best of --host-reps).  Cases: 10 / 30 / 60
masks at 1024^2 and 30 masks at 4096^2 (--cases n:size,...).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from saber_amd.filters import masks as fm  # noqa: E402
from saber_amd.filters._context import handle  # noqa: E402


def disc_masks(n, size, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:size, :size]
    out = []
    for _ in range(n):
        cy, cx = rng.integers(0, size, 2)
        r = int(rng.integers(size // 50, size // 9))
        out.append({"segmentation": (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r})
    return out, rng.uniform(0.34, 1.0, n).astype(np.float32)


def wall(fn, reps, sync):
    ms = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10:1024,30:1024,60:1024,30:4096", help="comma-separated masks:size")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--skip-host", action="store_true", help="device timings only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "consensus_bench measures on the device: there is no CPU fallback"
    eng = handle(0)
    res = {"cases": []}
    for case in args.cases.split(","):
        n, size = (int(v) for v in case.split(":"))
        masks, conf = disc_masks(n, size)
        shape = (size, size)
        row = {"masks": n, "size": size}
        if not args.skip_host:
            state = {}
            row["host"] = wall(lambda: state.update(out=fm._consensus_based_resolution(shape, masks, conf)), args.host_reps, False)
        stack = torch.from_numpy(np.stack([m["segmentation"] for m in masks]).astype(np.uint8)).cuda()
        dev_out = fm._consensus_based_resolution(shape, masks, conf, device=0)                    # warm-up: code object, workspace, allocator
        row["components"] = len(dev_out)
        reps = args.reps if size <= 2048 else max(2, args.reps // 3)
        row["box_upload"] = wall(lambda: fm._consensus_based_resolution(shape, masks, conf, device=0), reps, True)
        row["box_resident"] = wall(lambda: fm._consensus_based_resolution(shape, masks, conf, device=0, masks_dev=stack), reps, True)
        row["engine"] = wall(lambda: eng.consensus_components(stack, range(n), conf), reps, True)
        if not args.skip_host:
            host_out = state["out"]
            row["same_components"] = len(host_out) == len(dev_out) and all(
                a["area"] == b["area"] and a["bbox"] == b["bbox"] and np.array_equal(a["segmentation"], b["segmentation"]) for a, b in zip(host_out, dev_out))
            row["max_score_diff"] = max([abs(a["predicted_iou"] - b["predicted_iou"]) for a, b in zip(host_out, dev_out)], default=0.0)
            row["host_over_box_upload"] = row["host"]["min_ms"] / row["box_upload"]["median_ms"]
            row["host_over_box_resident"] = row["host"]["min_ms"] / row["box_resident"]["median_ms"]
        res["cases"].append(row)
        del stack, dev_out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
