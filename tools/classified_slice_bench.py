"""One classifier-filtered 1024^2 slice on the two routes of propagationSegmenter (saber_amd/segmenters/propagation.py):
    host    slice_by_slice: masks unpacked to numpy dicts, Predictor.batch_predict on the uploaded uint8 stack, numpy / scipy consensus
            resolution, numpy paint loop, scipy 3-D stitch (also the only route a classifier had before the device route looked at it)
    device  slice_by_slice_device: the generator's bit-packed rows all the way (Predictor.batch_predict_bits,
            Engine.consensus_components_bits, Engine.relabel_plane), stitch on the device
Model: Hiera-L with the seeded encoder and the fitted mask decoder (the synthetic weights whose IoU / stability filters bite), cfgAMG
defaults (32 x 32 points, 2 crop layers), a seeded 3-class head.  --bias lists values added to the head's class-1 bias: 0 is the head as
seeded, 10 makes every mask that passes the crop-area filter class 1 (the consensus and paint stages then see every mask).
Wall clock (time.perf_counter around a call that ends in a device synchronise) after --warmup calls of each route, the two routes
alternating, median and minimum over --reps.  The volume has one slice, so both routes run one slice on one handle.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--bias", default="0,10", help="comma-separated values added to classifier.4.bias[1] of the seeded head")
    ap.add_argument("--trunk", default="large")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "classified_slice_bench measures on the device: there is no CPU fallback"
    os.environ.setdefault("SABER_AMD_SEEDED_WEIGHTS", "fitted")
    from oracle import classifier_ref as cr
    from oracle import saber_ref
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.amg import cfgAMG
    from saber_amd.adapters.sam2.automask import get_engine
    from saber_amd.classifier.models.predictor import Predictor
    from saber_amd.segmenters.propagation import propagationSegmenter
    from saber_amd.segmenters.slice_driver import segment_slice_to_plane, select_masks

    amg = cfgAMG(sam2_cfg=args.trunk)
    eng = get_engine(args.trunk, "cuda:0")
    vol = saber_ref.synthetic_slice(seed=0, size=args.size)[None].astype(np.float32)
    res = {"size": args.size, "trunk": args.trunk, "weights": os.environ["SABER_AMD_SEEDED_WEIGHTS"], "reps": args.reps, "cases": []}
    for bias in (float(v) for v in args.bias.split(",")):
        Wh = {k: v.copy() for k, v in cr.seeded_head(3, 0).items()}
        Wh["classifier.4.bias"][1] += bias
        config = {"model": {"num_classes": 3}, "amg_params": {"sam2_cfg": args.trunk}}
        pred = Predictor(None, None, config=config, head_weights=Wh, engine=eng)
        seg = propagationSegmenter(deviceID=0, cfg=SAM2AdapterConfig(cfg=args.trunk, amg_cfg=amg, classifier=pred), min_mask_area=50)
        routes = {"host": lambda: seg.slice_by_slice(vol), "device": lambda: seg.slice_by_slice_device(vol)}
        out = {}
        for _ in range(args.warmup):
            for name, fn in routes.items():
                out[name] = fn()
        ms = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        # the counts behind the timings: masks the generator made, masks the classifier saw, masks of class 1, painted components
        gen = seg.adapter._generator()
        raw = torch.from_numpy(vol[0]).cuda()
        bits, meta = eng.amg_generate(eng.prepare(raw), gen.base_generator.params, max_masks=gen.base_generator.max_masks)
        H, W = raw.shape
        rows = select_masks(meta, eng.pair_intersections(bits, H, W).cpu().numpy(), seg.min_mask_area)
        probs = pred.batch_predict_bits(raw, bits, rows, W)
        plane, painted = segment_slice_to_plane(eng, raw, gen.base_generator.params, min_mask_area=seg.min_mask_area, classifier=pred,
                                                target_class=1, classifier_min_area=seg.batchsize)
        row = {"bias": bias, "masks_generated": len(meta), "masks_to_classifier": len(rows), "masks_classified": int((probs.sum(axis=1) > 0).sum()),
               "masks_of_class_1": int(((probs.argmax(axis=1) == 1) & (probs.sum(axis=1) > 0)).sum()), "components_painted": painted,
               "same_volume": bool(np.array_equal(out["host"], out["device"])), "labels": int(out["device"].max())}
        for name in routes:
            row[name] = {"median_ms": statistics.median(ms[name]), "min_ms": min(ms[name]), "max_ms": max(ms[name])}
        row["host_over_device"] = row["host"]["median_ms"] / row["device"]["median_ms"]
        res["cases"].append(row)
        pred.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
