"""Time of the hole-filling launch sequence (saber_k_fill_holes, csrc/holefill.hip) on 256 x 256 planes of speckled logits: the median of
HIP-event timings over `--reps` calls after warm-up, at 1 and 16 planes (one tracked object; the objects of a frame in one call).
    python tools/fill_holes_bench.py [--reps 200] [--planes 1 16]
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def speckled_logits(planes, seed=0, side=256):
    """smooth noise with 3 % sprinkled negative pixels: a few thousand background components per plane, most of them small"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    x = np.stack([ndimage.uniform_filter(p, 5) for p in rng.standard_normal((planes, side, side))]) * 10 + 1
    holes = rng.random(x.shape) < 0.03
    x[holes] = -np.abs(x[holes]) - 0.5
    return x.astype(np.float32)


def run(planes_list=(1, 16), reps=200, warmup=20, max_area=8):
    from saber_amd import _lib
    lib = _lib.load()
    assert torch.cuda.is_available(), "needs a ROCm device"
    if lib.saber_k_init(0) != 0:
        raise RuntimeError(lib.saber_k_last_error().decode())
    out = {"what": f"saber_k_fill_holes, 256x256 planes, max_area {max_area}: median / min / max of {reps} HIP-event timings after {warmup} warm-up calls",
           "cases": {}}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for planes in planes_list:
        x = torch.from_numpy(speckled_logits(planes)).cuda()
        y = torch.empty_like(x)
        ws = torch.empty(x.numel() * 8, dtype=torch.uint8, device="cuda")

        def call():
            if lib.saber_k_fill_holes(C.c_void_p(x.data_ptr()), planes, 256, 256, max_area, 0.1, C.c_void_p(y.data_ptr()), C.c_void_p(ws.data_ptr()),
                                      ws.numel(), stream) != 0:
                raise RuntimeError(lib.saber_k_last_error().decode())

        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        # back to back: what a caller that does not wait between calls pays per call
        n = reps
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        e1.synchronize()
        out["cases"][str(planes)] = {"median_us": round(float(np.median(ms)) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2),
                                     "back_to_back_us_per_call": round(e0.elapsed_time(e1) / n * 1e3, 2),
                                     "pixels_filled": int((y != x).sum().item())}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--planes", type=int, nargs="+", default=[1, 16])
    a = ap.parse_args()
    print(json.dumps(run(tuple(a.planes), a.reps)))
