"""The video path with SEVERAL propagations over one volume (tools/video_bench.py runs one): SAM2Adapter.set_volume once, then
segment_volume + reset_state from S seed frames - what propagationSegmenter does per seed slice and multiDepthTomoSegmenter per slab - on
the synthetic tomogram of that tool (Hiera-L, seeded weights with the +3 object-score bias, num_maskmem = 2, 32 frames of 256 x 256, 16
frames per encoder pass, forward + backward over the whole stack), with n disc seeds, on ONE handle, on two routes:
    off   every window is encoded (VideoPredictor(frame_store_gb=0))
    on    the frame-feature store: a frame goes through the encoder once per volume (frame_store_gb=1; dropped before every run, so that a
          run pays for its own encodes and exports)
With n > 1 both routes track the objects of a frame together (batch_objects).  Per (S, n) every route runs once as a warm-up, then the timed
runs ALTERNATE within the process (off, on, off, on: --repeats 2), so that the run-to-run spread is visible next to the difference.
    python tools/video_seeds_bench.py [--seeds 1,3] [--objects 1,4] [--precision fp16] [--out profiles/video_frame_store.json]
Per (route, S, n): ms per seed-frame = wall clock of a run / (S * frames) (the minimum of the timed runs, and every run), and the frames a
run sent through the encoder / copied from the store.  Prints one JSON line and writes the same to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seeds_for(n, size):
    """n discs on a grid that fills the frame (as tools/video_objects_bench.py)"""
    side = int(np.ceil(np.sqrt(n)))
    yy, xx = np.mgrid[:size, :size]
    pitch = size / side
    out = []
    for i in range(n):
        cy, cx = (i // side + 0.5) * pitch, (i % side + 0.5) * pitch
        out.append(((yy - cy) ** 2 + (xx - cx) ** 2 < (pitch / 3) ** 2).astype(np.float32))
    return out


def seed_frames(S, frames):
    """S seed frames spread over the stack: the middle frame for S = 1"""
    return [(i + 1) * frames // (S + 1) for i in range(S)]


def run(seeds=(1, 3), objects=(1, 4), trunk="large", frames=32, size=256, window=16, precision=None, repeats=2):
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
    vps = {"off": VideoPredictor(eng, W, num_maskmem=2, frame_store_gb=0), "on": VideoPredictor(eng, W, num_maskmem=2, frame_store_gb=1)}
    tomo = np.random.default_rng(42).uniform(-1, 1, (frames, size, size)).astype(np.float32)
    ad = SAM2Adapter(SAM2AdapterConfig(cfg=trunk), device="cuda:0")
    rows = []
    for S in seeds:
        starts = seed_frames(S, frames)
        for n in objects:
            masks = seeds_for(n, size)
            kw = {"batch_objects": True} if n > 1 else {}

            def once(route):
                vp = ad._video_predictor = vps[route]
                vp.drop_frame_store()                                       # a run is a new volume to the store
                enc, res = vp.encoded_frames, vp.restored_frames
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ad.set_volume(tomo)
                vols = []
                for start in starts:
                    vols.append(ad.segment_volume(start, masks=masks, min_presence_score=0.0, **kw))
                    ad.reset_state()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, vols, vp.encoded_frames - enc, vp.restored_frames - res

            check = {route: once(route) for route in ("off", "on")}         # warm-up: allocator, workspaces, lazy tables, the store's rows
            same = all(np.array_equal(a, b) for a, b in zip(check["off"][1], check["on"][1]))
            timed = {"off": [], "on": []}
            for _ in range(repeats):
                for route in ("off", "on"):                                 # alternating: a drift of the machine hits both routes alike
                    timed[route].append(once(route)[0])
            for route in ("off", "on"):
                per = [v / (S * frames) * 1e3 for v in timed[route]]
                rows.append({"seed_frames": S, "objects": n, "route": route, "ms_per_seed_frame": round(min(per), 3),
                             "ms_per_seed_frame_runs": [round(v, 3) for v in per], "encoded_frames_per_run": check[route][2],
                             "restored_frames_per_run": check[route][3], "volumes_equal_to_off": bool(same),
                             "labels": int(len(np.unique(check[route][1][0])) - 1)})
    store_bytes = vps["on"].store_bytes
    eng.close()
    return {"what": f"SAM2Adapter.set_volume once + S x (segment_volume + reset_state), {trunk} trunk, {getattr(eng, 'operands', 'bf16')} operands, {window} frames per "
                    f"encoder pass, {frames} frames of {size}x{size}, num_maskmem 2, forward + backward over the whole stack, n disc seeds (batch_objects "
                    f"with n > 1); per (S, n) one warm-up run per route, then {repeats} timed runs per route, alternating; ms_per_seed_frame = run / "
                    f"(S * frames), the fastest; the store is dropped before every run",
            "store_bytes": store_bytes, "rows": rows}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="1,3", help="numbers of seed frames per volume")
    ap.add_argument("--objects", default="1,4")
    ap.add_argument("--repeats", type=int, default=2, help="timed runs per route, alternating between the routes")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--trunk", default="large")
    ap.add_argument("--precision", default=None, help="engine precision (default: the engine's own, bf16)")
    ap.add_argument("--out", default=None, help="default: profiles/video_frame_store.json (video_frame_store_<precision>.json with --precision)")
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", f"video_frame_store{'_' + a.precision if a.precision else ''}.json")
    res = run(tuple(int(v) for v in a.seeds.split(",")), tuple(int(v) for v in a.objects.split(",")), a.trunk, a.frames, precision=a.precision,
              repeats=a.repeats)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
