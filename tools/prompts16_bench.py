"""Time per prompt of saber_decode_prompts on its three routes: the 8-token route (one point per prompt), the 16-token route of the 16-bit
kernels (saber_engine_set_multipoint; K = 2 and K = 9 points per prompt) and the exact precision mode (K = 2).

One Hiera-L handle (precision="exact", operands="fp16", max_prompts=1024, multipoint on), one encoded image; batches of n = 1 and
n = max_prompts / 2 prompts.  HIP events around each call, warm-up, median of --reps runs.  Prints one JSON line per measurement.

    python tools/prompts16_bench.py [--reps 20] [--exact-reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--exact-reps", type=int, default=20, help="runs of the exact mode (slow at n = 512)")
    ap.add_argument("--max-prompts", type=int, default=1024)
    a = ap.parse_args()
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import seeded_weights
    W = seeded_weights(get_config("large"), 0)
    eng = Engine("large", device=0, weights=W, max_images=1, max_prompts=a.max_prompts, precision="exact", operands="fp16", multipoint=True)
    eng.set_precision("fp16")
    img = torch.from_numpy(np.random.default_rng(0).uniform(0, 1, (1024, 1024)).astype(np.float32)).cuda()
    eng.encode(img)
    rng = np.random.default_rng(1)

    def timed(precision, n, k, reps):
        pts = torch.from_numpy(rng.uniform(0, 1024, (n, k, 2)).astype(np.float32)).cuda()
        lab = torch.ones(n, k, dtype=torch.int32, device="cuda")
        if k >= 2:
            lab[:, :2] = torch.tensor([2, 3], dtype=torch.int32)
        eng.set_precision(precision)
        for _ in range(a.warmup):
            eng.decode_prompts(pts, lab, slot=0, multimask=False)
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.decode_prompts(pts, lab, slot=0, multimask=False)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = float(np.median(ts))
        r = {"route": {1: "8-token"}.get(k, "16-token") if precision != "exact" else "exact", "precision": precision, "points": k, "n": n,
             "ms": round(ms, 4), "us_per_prompt": round(1000.0 * ms / n, 3), "runs": reps}
        print(json.dumps(r), flush=True)
        return r

    res = {}
    for n in (1, a.max_prompts // 2):
        res[("8", n)] = timed("fp16", n, 1, a.reps)
        res[("16k2", n)] = timed("fp16", n, 2, a.reps)
        res[("16k9", n)] = timed("fp16", n, 9, a.reps)
        res[("exact", n)] = timed("exact", n, 2, a.exact_reps)
    n = a.max_prompts // 2
    print(json.dumps({"n": n, "t16_over_t8": round(res[("16k2", n)]["ms"] / res[("8", n)]["ms"], 3),
                      "exact_over_t16": round(res[("exact", n)]["ms"] / res[("16k2", n)]["ms"], 3)}), flush=True)
    eng.check_finite()
    eng.close()


if __name__ == "__main__":
    main()
