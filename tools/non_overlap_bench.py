"""Time of the non-overlapping-masks output step of the video path on n planes of 256 x 256 logits resized to 1024 x 1024: the fused entry
(saber_k_resize_planes_non_overlap, csrc/video_ops.hip) against the two-step route that gives the same bits - saber_k_resize_plane of the n
planes, then upstream's torch formula (argmax, where, clamp) on the device.  Median of HIP-event timings over `--reps` calls after warm-up.
    python tools/non_overlap_bench.py [--reps 200] [--planes 2 8 32]
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def smooth_logits(planes, seed=0, side=256):
    """smooth noise around zero: every plane has large positive and negative regions, so planes overlap on about half of the pixels"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    return (np.stack([ndimage.uniform_filter(p, 9) for p in rng.standard_normal((planes, side, side))]) * 60).astype(np.float32)


def torch_constraint(x):
    """SAM2Base._apply_non_overlapping_constraints on (n, 1, H, W)"""
    if x.size(0) == 1:
        return x
    keep = torch.argmax(x, dim=0, keepdim=True) == torch.arange(x.size(0), device=x.device)[:, None, None, None]
    return torch.where(keep, x, torch.clamp(x, max=-10.0))


def timed(call, reps, warmup):
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
    return {"median_us": round(float(np.median(ms)) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2)}


def run(planes_list=(2, 8, 32), reps=200, warmup=20, side=256, out_side=1024):
    from saber_amd import _lib
    lib = _lib.load()
    assert torch.cuda.is_available(), "needs a ROCm device"
    if lib.saber_k_init(0) != 0:
        raise RuntimeError(lib.saber_k_last_error().decode())
    out = {"what": f"{side}x{side} -> {out_side}x{out_side} logits with the non-overlapping constraint: median / min / max of {reps} HIP-event timings "
                   f"after {warmup} warm-up calls; fused = saber_k_resize_planes_non_overlap, two_step = saber_k_resize_plane + the torch formula",
           "cases": {}}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in planes_list:
        x = torch.from_numpy(smooth_logits(n, side=side)).cuda()
        fused = torch.empty((n, out_side, out_side), device="cuda")
        plain = torch.empty_like(fused)
        held = {}

        def call_fused():
            if lib.saber_k_resize_planes_non_overlap(C.c_void_p(x.data_ptr()), n, side, side, C.c_void_p(fused.data_ptr()), out_side, out_side, -10.0, stream) != 0:
                raise RuntimeError(lib.saber_k_last_error().decode())

        def call_resize():
            if lib.saber_k_resize_plane(C.c_void_p(x.data_ptr()), n, side, side, C.c_void_p(plain.data_ptr()), out_side, out_side, 0, 0, 0.0, 0.0, stream) != 0:
                raise RuntimeError(lib.saber_k_last_error().decode())

        def call_two_step():
            call_resize()
            held["out"] = torch_constraint(plain[:, None])

        case = {"fused": timed(call_fused, reps, warmup), "two_step": timed(call_two_step, reps, warmup), "resize_alone": timed(call_resize, reps, warmup)}
        torch.cuda.synchronize()
        case["bit_equal"] = bool(torch.equal(fused.view(torch.int32), held["out"][:, 0].contiguous().view(torch.int32)))
        case["pixels_suppressed"] = int((fused != plain).sum().item())
        case["output_mib"] = round(fused.numel() * 4 / 2 ** 20, 1)
        case["speedup"] = round(case["two_step"]["median_us"] / case["fused"]["median_us"], 2)
        out["cases"][str(n)] = case
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--planes", type=int, nargs="+", default=[2, 8, 32])
    a = ap.parse_args()
    print(json.dumps(run(tuple(a.planes), a.reps)))
