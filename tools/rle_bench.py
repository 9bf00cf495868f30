"""Time of the mask generator's run-length output (csrc/rle.hip) on a 1024 x 1024 stack of n disc masks (default 227, the mask count of the
default-grid golden).  Per n:
  * the device time of saber_k_rle_count (three launches, back to back, device events) and of a count + encode pair (the pair includes the
    gap of the encode's capacity check, which waits for the count), with the GB/s of the pair against the bytes of the stack read twice;
    per-kernel times come from a profiler run of `--step` (rocprofv3 --kernel-trace --stats), not from here;
  * the host time of generate()'s tail, bits -> what goes under "segmentation": the RLE route (Engine.rle_encode + rle_dicts) and the
    bool-array route (unpack_bits), median / min / max over `--reps` runs each, alternating, after warm-up; bytes over the bus of each.
    python tools/rle_bench.py [--reps 20] [--n 227]
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


def stack(n, side=1024, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:side, :side].astype(np.float32)
    out = np.zeros((n, side, side), bool)
    for i in range(n):
        cy, cx = rng.uniform(0.1, 0.9, 2) * side
        r = rng.uniform(0.03, 0.3) * side
        out[i] = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return out


def step(n, reps, warmup, side=1024):
    import ctypes as C
    import numpy as np
    import torch
    from saber_amd.adapters.sam2.rle import rle_dicts
    from saber_amd.engine import Engine, unpack_bits
    assert torch.cuda.is_available(), "needs a ROCm device"
    eng = Engine.bare(0)
    lib = eng.lib
    masks = stack(n, side)
    W32 = side // 32
    words = np.packbits(masks, axis=-1, bitorder="little").view(np.uint32).reshape(n, side, W32)
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())

    # the two routes of generate()'s tail, alternating
    def tail_rle():
        counts, offsets = eng.rle_encode(bits, side)
        return rle_dicts(counts, offsets, side, side)

    def tail_bool():
        return unpack_bits(bits, side)

    ms = {"rle": [], "bool": []}
    entries = 0
    for r in range(warmup + reps):
        for name, fn in (("rle", tail_rle), ("bool", tail_bool)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            t1 = time.perf_counter()
            if r >= warmup:
                ms[name].append((t1 - t0) * 1e3)
            if name == "rle":
                entries = sum(len(d["counts"]) for d in out)
            del out

    # the kernels on the null stream: count alone, then count + encode pairs
    need = int(lib.saber_k_rle_workspace_bytes(n, side, side))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    assert lib.saber_k_rle_count(p(bits), n, side, side, p(offsets), p(ws), need, None) == 0, lib.saber_k_last_error()
    total = int(offsets[n].item())
    counts = torch.empty(total, dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        assert lib.saber_k_rle_count(p(bits), n, side, side, p(offsets), p(ws), need, None) == 0
    e1.record()
    e1.synchronize()
    count_ms = e0.elapsed_time(e1) / reps
    e0.record()
    for _ in range(reps):
        assert lib.saber_k_rle_count(p(bits), n, side, side, p(offsets), p(ws), need, None) == 0
        assert lib.saber_k_rle_encode(p(bits), n, side, side, p(offsets), p(counts), total, p(ws), need, None) == 0, lib.saber_k_last_error()
    e1.record()
    e1.synchronize()
    pair_ms = e0.elapsed_time(e1) / reps
    stack_bytes = n * side * W32 * 4
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"n": n, "run_lengths": entries, "stack_bytes": stack_bytes,
           "count_device_ms": round(count_ms, 4), "count_encode_device_ms": round(pair_ms, 4),
           "count_encode_GBps_stack_read_twice": round(2 * stack_bytes / (pair_ms * 1e-3) / 1e9, 1),
           "tail_rle_ms": {"median": round(med["rle"], 3), "min": round(min(ms["rle"]), 3), "max": round(max(ms["rle"]), 3)},
           "tail_bool_ms": {"median": round(med["bool"], 3), "min": round(min(ms["bool"]), 3), "max": round(max(ms["bool"]), 3)},
           "tail_speedup": round(med["bool"] / med["rle"], 1),
           "bus_bytes_rle": total * 4 + (n + 1) * 8 + 8, "bus_bytes_bool": n * side * side, "workspace_bytes": need}
    eng.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, nargs="+", default=[227])
    ap.add_argument("--step", type=int, default=None, help="(internal) measure this n in this process")
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps(step(a.step, a.reps, a.warmup)))
        sys.exit(0)
    out = {"what": f"run-length output at 1024x1024: device ms of the kernels and host ms of generate()'s tail (bits -> segmentation values), median of "
                   f"{a.reps} runs after {a.warmup} warm-up runs", "cases": []}
    for n in a.n:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(n), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            out["error"] = f"n = {n}: no result within {STEP_LIMIT_S} s"
            break
        if r.returncode != 0:
            out["error"] = f"n = {n}: exit status {r.returncode}: {r.stderr[-400:]}"
            break
        out["cases"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    sys.exit(1 if "error" in out else 0)
