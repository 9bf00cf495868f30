"""Slab preparation of tomoSegmenter.segment_vol, host route against device route, on the same synthetic tomogram:
    host    gaussian_smoothing_z (scipy correlate1d) -> preprocess.normalize (numpy) -> preprocess.project_tomogram (numpy)
    device  upload -> saber_k_correlate1d_zero with fused min / max -> saber_k_normalize_minmax in place -> saber_k_project_mean
Host steps: wall clock (time.perf_counter), best of --host-reps.  Device steps: device events around each step, after a warm-up pass,
median and minimum over --reps; the upload is a host clock around a copy that ends in a synchronise.  GB/s of the two whole-volume passes
are the bytes the algorithm needs (smoothing: the input once + the fp32 output once; normalise: 4 bytes read + 4 written per voxel) over
the median time, to be read next to the 6.29 TB/s of a float4 copy on this device.  --chunks sweeps the chunk_len argument of the
smoothing kernel (0 = the kernel's own choice).  Prints one JSON line."""
import argparse
import json
import statistics
import sys
import time
import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from saber_amd.segmenters.tomo import gaussian_smoothing_z  # noqa: E402
from saber_amd.utils import preprocessing as preprocess  # noqa: E402
from saber_amd.utils import volprep  # noqa: E402

COPY_TBS = 6.29


def synthetic(Z, S, dtype, seed=0):
    rng = np.random.default_rng(seed)
    plane = rng.normal(32768, 3000, (S, S)).astype(np.float32)
    vol = np.empty((Z, S, S), dtype=np.float32)
    for z in range(Z):                                   # a cheap z dependence: the planes differ, the generator runs once
        np.add(np.roll(plane, 17 * z, axis=1), np.float32(40.0 * np.sin(z / 9.0)), out=vol[z])
    return np.clip(vol, 0, 65535).astype(dtype)


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--z", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dtype", default="float32", choices=["float32", "int16", "uint16", "uint8"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--chunks", default="0", help="comma-separated chunk_len values for the smoothing kernel")
    ap.add_argument("--thickness", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true", help="device steps only (kernel A/Bs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "slab_prep_bench measures on the device: there is no CPU fallback"
    Z, S = args.z, args.size
    vol = synthetic(Z, S, np.dtype(args.dtype))
    n = vol.size
    taps = volprep.make_gaussian_kernel(5)
    zs = Z // 2
    res = {"shape": [Z, S, S], "dtype": args.dtype, "voxels": n}

    host = {"smooth_ms": [], "normalize_ms": [], "project_ms": []}
    for _ in range(0 if args.skip_host else args.host_reps):
        t0 = time.perf_counter()
        sm = gaussian_smoothing_z(vol, 5, dim=0)
        t1 = time.perf_counter()
        nv = preprocess.normalize(sm)
        t2 = time.perf_counter()
        img = preprocess.project_tomogram(nv, zs, args.thickness)
        t3 = time.perf_counter()
        host["smooth_ms"].append((t1 - t0) * 1e3)
        host["normalize_ms"].append((t2 - t1) * 1e3)
        host["project_ms"].append((t3 - t2) * 1e3)
        del sm
    if not args.skip_host:
        res["host_ms"] = {k[:-3]: min(v) for k, v in host.items()}
        res["host_ms"]["total"] = sum(res["host_ms"].values())

    dev = torch.device("cuda", 0)
    up = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tv = volprep.to_device_volume(vol, dev)
        torch.cuda.synchronize()
        up.append((time.perf_counter() - t0) * 1e3)
    res["upload_ms"] = {"median_ms": statistics.median(up), "min_ms": min(up), "what": "pageable host memory, one copy"}

    state = {}

    def smooth(chunk):
        state["s"], state["mm"] = volprep.correlate1d_zero(tv, taps, dim=0, minmax=True, chunk_len=chunk)

    smooth_bytes = n * (vol.dtype.itemsize + 4)
    res["smooth"] = {}
    for chunk in [int(c) for c in args.chunks.split(",")]:
        smooth(chunk)                                    # warm-up: code object, allocator
        torch.cuda.synchronize()
        r = timed(lambda: smooth(chunk), args.reps)
        r["GBps"] = smooth_bytes / r["median_ms"] / 1e6
        r["frac_of_copy_rate"] = r["GBps"] / (COPY_TBS * 1e3)
        res["smooth"][f"chunk_len={chunk}"] = r
    smooth(0)
    torch.cuda.synchronize()
    S0 = state["s"].clone()
    mm = state["mm"]

    def norm():
        volprep.normalize_minmax_(state["s"], mm)        # in place; repeated passes re-normalise the same buffer: same traffic, same arithmetic

    norm()
    torch.cuda.synchronize()
    r = timed(norm, args.reps)
    r["GBps"] = 8 * n / r["median_ms"] / 1e6
    r["frac_of_copy_rate"] = r["GBps"] / (COPY_TBS * 1e3)
    res["normalize"] = r
    state["s"].copy_(S0)
    del S0
    norm()
    dv = state["s"]
    preprocess.project_tomogram(dv, zs, args.thickness)
    torch.cuda.synchronize()
    res["project"] = timed(lambda: preprocess.project_tomogram(dv, zs, args.thickness), args.reps)

    def whole():
        s, m = volprep.correlate1d_zero(tv, taps, dim=0, minmax=True)
        volprep.normalize_minmax_(s, m)
        return preprocess.project_tomogram(s, zs, args.thickness)

    whole()
    torch.cuda.synchronize()
    res["device_prep_ms"] = timed(whole, args.reps)
    if args.skip_host:
        print(json.dumps(res))
        return
    dev_total = res["device_prep_ms"]["median_ms"]
    res["speedup_vs_host"] = {"kernels_only": res["host_ms"]["total"] / dev_total,
                              "with_upload": res["host_ms"]["total"] / (dev_total + res["upload_ms"]["median_ms"])}
    # same results: the device's normalised volume and slab image against the host route's
    dimg = whole().cpu().numpy()
    res["check"] = {"volume_max_abs_diff": float(np.abs(dv.cpu().numpy() - nv).max()), "image_max_abs_diff": float(np.abs(dimg - img).max())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
