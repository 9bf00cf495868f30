"""Time of the mask generator's small-region step on an engine handle (saber_amg_postprocess_small_regions, csrc/smallregions.hip) on
1024 x 1024 stacks of n = 29 and n = 227 masks (the mask counts of the fitted and the default-grid goldens): groups of a clean ellipse, a
noisy copy of it and two noisy copies of a second one, the recipe of tests/small_regions_ref.py:random_stack.  Per n: median / min / max of the
host time of a call (it ends with the call's one synchronisation) over `--reps` calls after warm-up, the effective bandwidth on the packed
rows it reads and writes, the label workspace and the staging the handle holds.
    python tools/small_regions_bench.py [--reps 10] [--n 29 227] [--min-area 25]
Every n is measured in a process of its own under its own time limit; a step that fails or runs out of time ends the run.
Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 240


def stack(n, side=1024, p=0.03, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:side, :side].astype(np.float32)
    out = np.zeros((n, side, side), bool)
    base = None
    for i in range(n):
        k = i % 4
        if k in (0, 2):
            cy, cx = rng.uniform(0.2, 0.8, 2) * side
            ry, rx = rng.uniform(0.12, 0.3, 2) * side
            base = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
        out[i] = base if k == 0 else base ^ (rng.random((side, side), dtype=np.float32) < p)
    return out


def step(n, reps, warmup, min_area, side=1024):
    import ctypes as C
    import numpy as np
    import torch
    from saber_amd import _lib
    from saber_amd.engine import Engine
    assert torch.cuda.is_available(), "needs a ROCm device"
    eng = Engine.bare(0)
    masks = stack(n, side)
    W32 = side // 32
    words = np.packbits(masks, axis=-1, bitorder="little").view(np.uint32).reshape(n, side, W32)
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    meta = [_lib.MaskMeta() for _ in range(n)]
    ms = []
    kept = 0
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, rec = eng.postprocess_small_regions(bits, meta, side, side, min_area, 0.7)
        t1 = time.perf_counter()
        kept = len(rec)
        if r >= warmup:
            ms.append((t1 - t0) * 1e3)
    # the clean-up kernels alone (no NMS, no compaction, no synchronisation inside), back to back
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.remove_small_regions(bits, side, min_area)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        _, changed, _, _ = eng.remove_small_regions(bits, side, min_area)
    e1.record()
    e1.synchronize()
    per = int(eng.lib.saber_k_mask_small_regions_bytes(side, side))
    med = float(np.median(ms))
    packed = 2 * n * side * W32 * 4
    res = {"n": n, "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
           "cleanup_kernels_ms": round(e0.elapsed_time(e1) / reps, 3),
           "effective_GBps_packed_rows": round(packed / (med * 1e-3) / 1e9, 2), "Mpixel_per_s": round(n * side * side / (med * 1e-3) / 1e6, 1),
           "masks_changed": int(changed.sum().item()), "masks_kept": kept,
           "workspace_bytes_per_mask": per, "label_workspace_bytes": per * max(1, min(n, (128 << 20) // per)),
           "staging_bytes": n * side * W32 * 4 + (7 * n + 1) * 4 + n * 64}
    eng.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, nargs="+", default=[29, 227])
    ap.add_argument("--min-area", type=int, default=25)
    ap.add_argument("--step", type=int, default=None, help="(internal) measure this n in this process")
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps(step(a.step, a.reps, a.warmup, a.min_area)))
        sys.exit(0)
    out = {"what": f"saber_amg_postprocess_small_regions at 1024x1024, min_area {a.min_area}, NMS 0.7: host ms per call (one synchronisation) over {a.reps} "
                   f"calls after {a.warmup} warm-up calls", "cases": []}
    for n in a.n:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(n), "--reps", str(a.reps), "--warmup", str(a.warmup),
                                "--min-area", str(a.min_area)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            out["error"] = f"n = {n}: no result within {STEP_LIMIT_S} s"
            break
        if r.returncode != 0:
            out["error"] = f"n = {n}: exit status {r.returncode}: {r.stderr[-400:]}"
            break
        out["cases"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    sys.exit(1 if "error" in out else 0)
