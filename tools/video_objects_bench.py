"""The video path with SEVERAL tracked objects (tools/video_bench.py tracks one): SAM2Adapter.set_volume + segment_volume on the synthetic
tomogram of that tool - Hiera-L, seeded weights with the +3 object-score bias, num_maskmem = 2, 32 frames of 256 x 256, forward + backward
from the middle frame - with n = 1, 4 and 16 disc seeds, on ONE handle, on three routes:
    off   object by object (batch_objects off)
    attn  the memory attention of a frame's objects as one batch, the rest of the frame per object (batch_objects on, batch_tail off)
    on    attention and tail batched: SAM heads enqueued for all objects, one host wait per frame, one memory encoder (batch_tail on: the default)
Per n every route runs once as a warm-up, then the timed runs ALTERNATE within the process (off, attn, on, off, attn, on: --repeats 2), so
that the run-to-run spread is visible next to the differences between the routes.
    python tools/video_objects_bench.py [--objects 1,4,16] [--routes off,attn,on] [--precision fp16] [--out profiles/video_objects_tail.json]
Per (route, n): ms per frame (the minimum of the timed runs, and every run), ms per object-frame, launches per frame of the engine's kernel
classes (eng.profile_begin / _end: encoder and SAM heads) and kernel-level C-ABI calls per frame (the memory path's saber_k_* calls, counted
on the host: one or two launches each).  Prints one JSON line and writes the same to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Counting:
    """the library handle of a VideoPredictor with its saber_k_* calls counted"""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("saber_k_") or name in ("saber_k_last_error", "saber_k_set_operand_type"):
            return fn

        def call(*a):
            self.calls += 1
            return fn(*a)
        return call


def seeds_for(n, size):
    """n discs on a grid that fills the frame"""
    side = int(np.ceil(np.sqrt(n)))
    yy, xx = np.mgrid[:size, :size]
    pitch = size / side
    out = []
    for i in range(n):
        cy, cx = (i // side + 0.5) * pitch, (i % side + 0.5) * pitch
        out.append(((yy - cy) ** 2 + (xx - cx) ** 2 < (pitch / 3) ** 2).astype(np.float32))
    return out


def run(objects=(1, 4, 16), routes=("off", "attn", "on"), trunk="large", frames=32, size=256, window=16, precision=None, repeats=2):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    from saber_amd.adapters.sam2.video import VideoPredictor
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import param_specs, seeded_weights
    cfg = get_config(trunk)
    W = seeded_weights(cfg, 0, video=True)
    k = "sam_mask_decoder.pred_obj_score_head.layers.2.bias"
    W[k] = W[k] + np.float32(3.0)
    img_keys = set(param_specs(cfg).keys())
    eng = Engine(trunk, device=0, weights={n: v for n, v in W.items() if n in img_keys}, max_images=window, max_prompts=8,
                 **({"precision": precision} if precision else {}))
    vp = VideoPredictor(eng, W, num_maskmem=2)
    tomo = np.random.default_rng(42).uniform(-1, 1, (frames, size, size)).astype(np.float32)
    ad = SAM2Adapter(SAM2AdapterConfig(cfg=trunk), device="cuda:0")
    ad._video_predictor = vp
    rows = []
    for n in objects:
        seeds = seeds_for(n, size)

        def once(route):
            kw = {} if route == "off" else {"batch_objects": True}          # "off" passes nothing: the route every earlier version has
            vp.batch_tail = route == "on"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ad.set_volume(tomo)
            vol = ad.segment_volume(frames // 2, masks=seeds, min_presence_score=0.0, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, vol

        for route in routes:
            once(route)                                                     # warm-up: allocator, workspaces, lazy tables
        timed = {route: [] for route in routes}
        for _ in range(repeats):
            for route in routes:                                            # alternating: a drift of the machine hits every route alike
                timed[route].append(once(route)[0])
        for route in routes:
            dt = min(timed[route])
            real_lib = vp.lib
            vp.lib = _Counting(real_lib)
            eng.profile_begin()
            try:
                _, vol = once(route)
            finally:
                prof = eng.profile_end()
                calls, vp.lib = vp.lib.calls, real_lib
            rows.append({"objects": n, "route": route, "ms_per_frame": round(dt / frames * 1e3, 3), "ms_per_object_frame": round(dt / frames / n * 1e3, 3),
                         "ms_per_frame_runs": [round(v / frames * 1e3, 3) for v in timed[route]],
                         "engine_launches_per_frame": round(sum(v["launches"] for v in prof.values()) / frames, 1),
                         "kernel_level_calls_per_frame": round(calls / frames, 1), "labels": int(len(np.unique(vol)) - 1),
                         "engine_kernel_classes_ms_per_frame": {c: round(v["ms"] / frames, 3) for c, v in prof.items() if v["launches"]}})
    eng.close()
    return {"what": f"SAM2Adapter.set_volume + segment_volume, {trunk} trunk, {eng.operands if hasattr(eng, 'operands') else 'bf16'} operands, {window} frames per encoder pass, "
                    f"{frames} frames of {size}x{size}, num_maskmem 2, forward + backward, n disc seeds on the middle frame; per n one warm-up run per route, "
                    f"then {repeats} timed runs per route, alternating; ms_per_frame = the fastest",
            "rows": rows}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", default="1,4,16")
    ap.add_argument("--routes", default="off,attn,on")
    ap.add_argument("--repeats", type=int, default=2, help="timed runs per route and n, alternating between the routes")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--trunk", default="large")
    ap.add_argument("--precision", default=None, help="engine precision (default: the engine's own, bf16)")
    ap.add_argument("--out", default=None, help="default: profiles/video_objects_tail.json (video_objects_tail_<precision>.json with --precision)")
    a = ap.parse_args()
    routes = tuple(a.routes.split(","))
    if not routes or any(r not in ("off", "attn", "on") for r in routes):
        ap.error("--routes takes off, attn and on")
    out = a.out or os.path.join(ROOT, "profiles", f"video_objects_tail{'_' + a.precision if a.precision else ''}.json")
    res = run(tuple(int(v) for v in a.objects.split(",")), routes, a.trunk, a.frames, precision=a.precision, repeats=a.repeats)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
