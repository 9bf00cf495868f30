"""Tail of a sliding-window micrograph run in both routes (saber_amd/segmenters/windows.py, csrc/windows.hip).

The generator runs once per window of a synthetic micrograph (default 4096 x 4096, window 1024 / overlap 0.25: 25 windows) and its
(bits, meta) pairs are kept on the device.  Timed, alternating, after warm-up, is everything BEHIND the generator up to the
filters.masks.masks_to_array stack on the host:
  * host route (saber2D.segment_image(use_sliding_window=True) + masks_to_array, device_windows = False): per window the unpack and download
    of every mask, the filters, duplicate removal and sort, then rasterize_masks and masks_to_array;
  * device route (windows.collect_windows + WindowMasks.to_array_host): filters from scalars, one intersection matrix per window, the
    survivors' rows gathered, the stack written from them in chunks and downloaded.
Both stacks are compared (they must be equal).  Then the two kernels alone, back to back between device events: achieved GB/s against their
traffic floors (place: n H W32 4 B written + the window words read; stack: count H W elem B written).
    SABER_AMD_SEEDED_WEIGHTS=fitted python tools/windows_bench.py [--size 4096] [--window 1024] [--overlap 0.25] [--reps 5] [--warmup 1]
Prints one JSON line.  Needs a ROCm device."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def micrograph(size, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    img = rng.normal(32768, 3000, (size, size)).astype(np.float32)
    yy, xx = np.mgrid[:size, :size].astype(np.float32)
    for _ in range(max(9, 40 * (size // 1024) ** 2)):
        cy, cx = rng.uniform(0.02, 0.98, 2) * size
        r = rng.uniform(15, 90)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += rng.choice([-6000.0, 6000.0])
    return np.clip(img, 0, 65535)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--window", type=int, default=1024)
    ap.add_argument("--overlap", type=float, default=0.25)
    ap.add_argument("--npoints", type=int, default=16)
    ap.add_argument("--crop-n-layers", type=int, default=0)
    ap.add_argument("--iou", type=float, default=0.7)
    ap.add_argument("--stability", type=float, default=0.92)
    ap.add_argument("--min-mask-area", type=int, default=50)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-reps", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "tools/windows_bench.py measures on a ROCm device; there is nothing to measure without one"
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.amg import cfgAMG
    from saber_amd.filters.masks import masks_to_array
    from saber_amd.segmenters import windows
    from saber_amd.segmenters.micro import cryoMicroSegmenter
    from saber_amd.utils import preprocessing

    amg = cfgAMG(npoints=a.npoints, crop_n_layers=a.crop_n_layers, pred_iou_thresh=a.iou, stability_score_thresh=a.stability, sam2_cfg="small")
    seg = cryoMicroSegmenter(deviceID=0, cfg=SAM2AdapterConfig(cfg="tiny", amg_cfg=amg, min_mask_area=a.min_mask_area), min_mask_area=a.min_mask_area,
                             window_size=a.window, overlap_ratio=a.overlap)
    img = micrograph(a.size)
    H, W = img.shape
    gen = seg.adapter._generator()
    base = gen.base_generator
    eng = base.engine
    wins = seg.get_sliding_windows(img.shape)
    t0 = time.perf_counter()
    with torch.inference_mode():
        generated = []
        for win in wins:
            window = img[win[0]:win[2], win[1]:win[3]]
            bits, meta = base.generate_device(preprocessing.prepare(window, to_rgb=True, engine=eng))
            generated.append((win, bits, meta))
    torch.cuda.synchronize()
    generator_s = time.perf_counter() - t0

    def host_tail():
        # saber2D.segment_image's sliding-window branch behind adapter.segment_image_2d's generator call, then segment_micrograph_core's stack
        collected = []
        for (y1, x1, y2, x2), bits, meta in generated:
            found = windows._wrapper_filters(gen, base._dicts(bits, meta, y2 - y1, x2 - x1), y2 - y1, x2 - x1)
            local = []
            for m in found:
                if m["area"] < seg.min_mask_area:
                    continue
                m["offset"] = (y1, x1)
                m["bbox"] = seg._to_global_bbox(m["bbox"], y1, x1)
                local.append(m)
            collected.extend(seg._apply_classifier(img[y1:y2, x1:x2], local))
        return masks_to_array(seg.rasterize_masks(img, collected)) if collected else np.zeros((0, H, W), np.uint8)

    def device_tail():
        wm = windows.collect_windows(gen, generated, H, W, seg.min_mask_area, seg.remove_repeating_masks)
        return wm, wm.to_array_host(chunk=a.chunk)

    ms = {"host": [], "device": []}
    equal, wm = None, None
    with torch.inference_mode():
        for r in range(a.warmup + a.reps):
            for name in ("host", "device"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = host_tail() if name == "host" else device_tail()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    ms[name].append(dt)
                if name == "host":
                    ref = out
                else:
                    wm, stack = out
                    if equal is None:
                        equal = bool(stack.dtype == ref.dtype and stack.shape == ref.shape and np.array_equal(stack, ref))
                    del stack
                del out
            del ref
    n = len(wm)
    res = {"what": f"tail of a sliding-window run behind the generator, up to the masks_to_array stack on the host: ms over {a.reps} runs after "
                   f"{a.warmup} warm-up run(s), the two routes alternating", "frame": [H, W], "window": a.window, "overlap": a.overlap,
           "windows": len(wins), "generated_masks": sum(len(m) for _, _, m in generated), "surviving_masks": n, "stacks_equal": equal,
           "generator_s_all_windows": round(generator_s, 2)}
    for k, v in ms.items():
        res[f"tail_{k}_ms"] = {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    res["tail_speedup"] = round(float(np.median(ms["host"]) / np.median(ms["device"])), 2)
    if n:
        W32 = (W + 31) // 32
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        bits = eng.place_window_masks(wm.src, wm.table_c, H, W)           # warm-up
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.kernel_reps):
            bits = eng.place_window_masks(wm.src, wm.table_c, H, W)
        e1.record()
        e1.synchronize()
        place_ms = e0.elapsed_time(e1) / a.kernel_reps
        place_bytes = n * H * W32 * 4 + int(wm.src.numel()) * 4
        del bits
        k = min(a.chunk, n)
        dev = eng.window_label_stack(wm.src, wm.table_c, H, W, first=0, count=k)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.kernel_reps):
            eng.window_label_stack(wm.src, wm.table_c, H, W, first=0, count=k, out=dev)
        e1.record()
        e1.synchronize()
        stack_ms = e0.elapsed_time(e1) / a.kernel_reps
        stack_bytes = k * H * W * dev.element_size()
        res["kernels"] = {"place": {"masks": n, "ms_per_call": round(place_ms, 4), "floor_bytes": place_bytes,
                                    "GBps": round(place_bytes / (place_ms * 1e-3) / 1e9, 1)},
                          "stack": {"planes": k, "elem_bytes": dev.element_size(), "ms_per_call": round(stack_ms, 4), "floor_bytes": stack_bytes,
                                    "GBps": round(stack_bytes / (stack_ms * 1e-3) / 1e9, 1)},
                          "note": "a call = the table upload and one launch, back to back between device events"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
