"""Time of the low-res clean-up launch (saber_k_clean_lowres, csrc/lowres_cleanup.hip) on 256 x 256 planes of speckled logits, as the mask
generator calls it: through an index map with pass flags, 64 / 1 024 / 9 216 planes (a group of first-pass candidates .. the m2m candidates of
a default slice) with 10 %, 50 % and 100 % of the flags set.  The call works in place, so every timed call starts from a fresh copy of the
planes (the copy is outside the timed interval); median of HIP-event timings over `--reps` calls after warm-up.
    python tools/lowres_cleanup_bench.py [--reps 20] [--planes 64 1024 9216] [--live 10 50 100] [--area 25] [--yardstick]
--yardstick adds saber_k_fill_holes (one polarity, through HBM: csrc/holefill.hip) on the same planes, all of them, at 64 and 1 024.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def speckled_logits(planes, seed=0, side=256, distinct=64):
    """smooth noise with 3 % of the pixels flipped in sign: thousands of components of both polarities per plane, most of them small;
    `distinct` planes are made on the host and repeated on the device"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    k = min(planes, distinct)
    x = np.stack([ndimage.uniform_filter(p, 7) for p in rng.standard_normal((k, side, side))]) * 12
    f = rng.random(x.shape) < 0.03
    x[f] = -x[f] - np.sign(x[f]) * 0.25
    base = torch.from_numpy(x.astype(np.float32)).cuda()
    return base.repeat((planes + k - 1) // k, 1, 1)[:planes].contiguous()


def timed(call, reset, reps, warmup):
    for _ in range(warmup):
        reset()
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_us": round(float(np.median(ms)) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2)}


def run(planes_list=(64, 1024, 9216), live_list=(10, 50, 100), reps=20, warmup=3, area=25, yardstick=False):
    from saber_amd import _lib
    lib = _lib.load()
    assert torch.cuda.is_available(), "needs a ROCm device"
    if lib.saber_k_init(0) != 0:
        raise RuntimeError(lib.saber_k_last_error().decode())
    out = {"what": f"saber_k_clean_lowres, 256x256 planes, both areas {area}, index map + pass flags: median / min / max of {reps} HIP-event timings "
                   f"after {warmup} warm-up calls, every call on a fresh copy", "cases": {}}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rng = np.random.default_rng(1)
    for planes in planes_list:
        x0 = speckled_logits(planes)
        x = torch.empty_like(x0)
        idx = torch.from_numpy(rng.permutation(planes).astype(np.int32)).cuda()
        for live in live_list:
            flags_h = np.zeros(planes, np.uint8)
            flags_h[rng.permutation(planes)[:max(1, planes * live // 100)]] = 1
            flags = torch.from_numpy(flags_h).cuda()

            def call():
                if lib.saber_k_clean_lowres(ptr(x), ptr(idx), ptr(flags), planes, 256, 256, 0.0, area, area, stream) != 0:
                    raise RuntimeError(lib.saber_k_last_error().decode())

            r = timed(call, lambda: x.copy_(x0), reps, warmup)
            n_live = int(flags_h.sum())
            r.update(live_planes=n_live, us_per_live_plane=round(r["median_us"] / n_live, 3),
                     gb_per_s_of_256KiB_per_live_plane=round(n_live * 262144 / (r["median_us"] * 1e-6) / 1e9, 1), pixels_changed=int((x != x0).sum().item()))
            out["cases"][f"{planes} planes, {live}% live"] = r
        if yardstick and planes <= 1024:
            y = torch.empty_like(x0)
            ws = torch.empty(x0.numel() * 8, dtype=torch.uint8, device="cuda")

            def call_fill():
                if lib.saber_k_fill_holes(ptr(x0), planes, 256, 256, area, 0.1, ptr(y), ptr(ws), ws.numel(), stream) != 0:
                    raise RuntimeError(lib.saber_k_last_error().decode())

            r = timed(call_fill, lambda: None, reps, warmup)
            r.update(us_per_plane=round(r["median_us"] / planes, 3))
            out["cases"][f"yardstick saber_k_fill_holes, {planes} planes (one polarity)"] = r
            del y, ws
        del x0, x
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--planes", type=int, nargs="+", default=[64, 1024, 9216])
    ap.add_argument("--live", type=int, nargs="+", default=[10, 50, 100])
    ap.add_argument("--area", type=int, default=25)
    ap.add_argument("--yardstick", action="store_true")
    a = ap.parse_args()
    print(json.dumps(run(tuple(a.planes), tuple(a.live), a.reps, area=a.area, yardstick=a.yardstick)))
