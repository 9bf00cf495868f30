#!/usr/bin/env python
"""Capture tests/golden/saber_membranes.npz: the reference's organelle / membrane refinement, run on the CPU over seeded scenes.

    python tools/make_golden_membranes.py /path/to/saber/analysis/refine_membranes.py

The reference module (torch, numpy, scipy, tqdm only) is loaded by path; nothing of it is copied.  On the CPU its opening goes through
scipy.ndimage.binary_opening, which is bit-identical on 0/1 volumes to the conv3d route it takes on a GPU, so these are the
expectations for the device pipeline.  Every condition a scene is meant to show is asserted while capturing.

Stored per run r<k>: organelle / membrane input (uint8), the two flattened output maps (uint8), a JSON record of the configuration,
the organelle input dtype, and the output's ndim / dtype / container.  For the small scene the 4-D stacks are stored too."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "saber_membranes.npz")


def load_reference(path):
    spec = importlib.util.spec_from_file_location("reference_refine_membranes", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def ellipsoid(shape, c, r):
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0


def shell(shape, c, r, out=1.0, inn=2.0):
    r = np.asarray(r, float)
    return ellipsoid(shape, c, r + out) & ~ellipsoid(shape, c, r - inn)


def extent(mask):
    idx = np.nonzero(mask)
    return [int(i.max() - i.min() + 1) for i in idx]


def main_scene():
    """(64,160,200): 1 round + interior membrane blob, 2 elongated, 3 without membrane, 4 too small, 5 with a y-extent of exactly
    24 = float32(0.15 * 160), 6 inside the trimmed z planes, 7 and 8 touching."""
    shape = (64, 160, 200)
    org = np.zeros(shape, np.uint8)
    mem = np.zeros(shape, bool)
    bodies = {1: ((32, 45, 50), (14, 20, 22)), 2: ((32, 45, 140), (5, 14, 40)), 3: ((32, 100, 30), (10, 14, 18)),
              4: ((32, 100, 70), (6, 6, 6)), 5: ((32, 100.5, 110), (10, 12, 18)), 7: ((32, 135, 120), (12, 14, 18)),
              8: ((32, 135, 156), (12, 14, 18))}
    for v, (c, r) in bodies.items():
        org[ellipsoid(shape, c, r)] = v
        if v != 3:
            mem |= shell(shape, c, r)
    org[0:5, 125:136, 20:41] = 6
    mem[0:5, 125:136, 18:43] = True
    blob = ellipsoid(shape, (32, 45, 50), (6, 6, 6))
    mem |= blob
    assert blob.sum() >= 500
    assert extent(org == 5)[1] == 24 and extent(org == 4)[1] < 24
    e2 = extent(org == 2)
    assert max(e2) + 4 > 3 * (min(e2) + 4), e2
    return org, mem.astype(np.uint8), blob


def small_scene():
    shape = (32, 64, 80)
    org = np.zeros(shape, np.uint8)
    mem = np.zeros(shape, bool)
    for v, (c, r) in {1: ((16, 20, 22), (8, 12, 14)), 2: ((16, 44, 56), (7, 11, 16)), 3: ((16, 48, 18), (6, 8, 9))}.items():
        org[ellipsoid(shape, c, r)] = v
        if v != 3:
            mem |= shell(shape, c, r)
    return org, mem.astype(np.uint8)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    d = ref.FilteringConfig()
    data = {"defaults": np.array(json.dumps({k: getattr(d, k) for k in ("ball_size", "min_membrane_area", "edge_trim_z", "edge_trim_xy",
                                                                        "min_roi_relative_size", "batch_size", "keep_surface_membranes")}))}
    runs = []

    def capture(org, mem, org_dtype, keep_stacks=False, as_torch=False, **cfg):
        f = ref.OrganelleMembraneFilter(ref.FilteringConfig(**cfg))           # no device here: the CPU route
        o_in = org.astype(org_dtype)
        if as_torch:
            res = f.run(torch.from_numpy(o_in), torch.from_numpy(mem), batch_processing=True)
        else:
            res = f.run(o_in, mem, batch_processing=True)
        o4, m4 = res["organelles"], res["membranes"]
        container = "torch" if isinstance(o4, torch.Tensor) else "numpy"
        assert str(o4.dtype).replace("torch.", "") == np.dtype(org_dtype).name and str(m4.dtype) == str(o4.dtype)
        ndim = o4.ndim
        if ndim == 4:
            o3, m3 = f.convert_to_3d_labels(o4), f.convert_to_3d_labels(m4)
        else:
            o3, m3 = o4, m4
        o4n, m4n, o3n, m3n = (np.asarray(a.numpy() if isinstance(a, torch.Tensor) else a) for a in (o4, m4, o3, m3))
        assert o3n.max(initial=0) < 256 and m3n.max(initial=0) < 256
        k = len(runs)
        rec = dict(cfg=cfg, org_dtype=np.dtype(org_dtype).name, ndim=int(ndim), container=container, as_torch=bool(as_torch),
                   n_pairs=int(o4n.shape[0]) if ndim == 4 else 0, stacks=bool(keep_stacks and ndim == 4))
        data[f"r{k}_org"], data[f"r{k}_mem"] = org.astype(np.uint8), mem.astype(np.uint8)
        data[f"r{k}_org_out"], data[f"r{k}_mem_out"] = o3n.astype(np.uint8), m3n.astype(np.uint8)
        if rec["stacks"]:
            data[f"r{k}_org_stack"], data[f"r{k}_mem_stack"] = o4n.astype(np.uint8), m4n.astype(np.uint8)
        runs.append(rec)
        return o4n, m4n, o3n, m3n

    org, mem, blob = main_scene()
    base = dict(min_membrane_area=500, edge_trim_z=5, edge_trim_xy=3, min_roi_relative_size=0.15)
    for ball_size in (3, 5):
        o4, m4, o3, m3 = capture(org, mem, np.uint8, ball_size=ball_size, keep_surface_membranes=False, **base)
        present = set(np.unique(o3).tolist()) - {0}
        assert {2, 3, 6, 8, 9} <= present, present                      # organelles 1, 2, 5, 7, 8 survive as 2, 3, 6, 8, 9
        assert not ({4, 5, 7} & present), present                       # 3: no membrane; 4: too small; 6: trimmed planes
        overlap = [(i, j) for i in range(len(m4)) for j in range(i + 1, len(m4)) if ((m4[i] > 0) & (m4[j] > 0)).any()]
        assert overlap, "no two refined membranes overlap: the overwrite order would not show"
        o4s, m4s, o3s, m3s = capture(org, mem, np.uint8, ball_size=ball_size, keep_surface_membranes=True, **base)
        assert (m3 != m3s).any() and (m3[blob] > 0).any() and not (m3s[blob] > 0).any(), "the interior blob does not show"
        print(f"ball {ball_size}: pairs {len(o4)}; membrane voxels {int((m3 > 0).sum())} -> {int((m3s > 0).sum())} (surface only); "
              f"organelle maps equal {bool((o3 == o3s).all())}; overlapping membrane pairs {overlap}")
    o4, m4, o3, m3 = capture(org, mem, np.uint8, ball_size=3, keep_surface_membranes=False, **dict(base, edge_trim_z=0))
    assert o4.ndim == 3 and not o4.any()                                # edge_trim_z = 0 empties everything: 3-D zeros
    capture(org, mem, np.int32, ball_size=3, keep_surface_membranes=False, **base)
    capture(org, mem, np.int64, ball_size=5, keep_surface_membranes=True, as_torch=True, **base)
    sorg, smem = small_scene()
    for ball_size in (3, 5):
        o4, m4, o3, m3 = capture(sorg, smem, np.uint8, keep_stacks=True, ball_size=ball_size, keep_surface_membranes=False,
                                 min_membrane_area=200, edge_trim_z=3, edge_trim_xy=2, min_roi_relative_size=0.15)
        assert o4.ndim == 4 and len(o4) >= 2
    data["runs"] = np.array(json.dumps(runs))
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, size
    print(f"wrote {OUT}: {len(runs)} runs, {size} bytes")


if __name__ == "__main__":
    main()
