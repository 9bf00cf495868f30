#!/usr/bin/env python
"""Record tests/golden/smooth_parent_bits.npz: the bytes Engine.smooth_labels and Engine.gaussian_smoothing_3d give on the MI355X for
the volumes of tests/smooth_parent_bits_cases.py.

    git checkout <the commit whose bytes are to be pinned> && python -c 'import __graft_entry__ as g; g.build()'
    python tools/record_smooth_bits.py [--out FILE]

Run it on the commit BEFORE a change to csrc/smooth3d.hip that claims the same summation order; tests/test_gpu_smooth_parent_bits.py then
holds the changed code to these bytes.  Outputs only (compressed): the test rebuilds the inputs from their seeds.  While recording,
every label of the two constructed volumes must set some voxel, the three element sizes of `deep` must agree, and the chunk route must give the same bytes."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import smooth_parent_bits_cases as cases  # noqa: E402
import sharded_smooth_ref as ref  # noqa: E402
from saber_amd.engine import Engine  # noqa: E402
from saber_amd.segmenters import smooth  # noqa: E402


def to_dev(vol):
    v = np.ascontiguousarray(vol)
    return torch.from_numpy(v.view({1: np.uint8, 2: np.int16, 4: np.int32}[v.dtype.itemsize])).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "smooth_parent_bits.npz"))
    args = ap.parse_args()
    eng = Engine.bare(0)
    rec = {}
    for name, (vol, scale) in cases.label_cases().items():
        dev = to_dev(vol)
        out, n = eng.smooth_labels(dev, scale)
        got = out.cpu().numpy()
        labels = np.unique(vol[vol != 0])
        assert n == labels.size and got.any(), name
        assert name.startswith("blob") or all((got == int(v)).any() for v in labels), name
        for parts in (1, 2, 3, vol.shape[0]):
            chunks = smooth.smooth_labels_chunks(eng, [dev[a:b] for a, b in ref.cuts_of(vol.shape[0], parts)], scale)
            assert torch.equal(torch.cat(chunks, 0), out), (name, parts)
        rec[name] = got
        print(f"{name}: {vol.shape} scale {scale}, {n} labels, {int((got != 0).sum())} voxels set of {int((vol != 0).sum())} labelled")
    vol, scale = cases.deep()
    for dt in (np.uint8, np.uint16):
        assert np.array_equal(eng.smooth_labels(to_dev(vol.astype(dt)), scale)[0].cpu().numpy(), rec["deep"]), dt
    field = eng.gaussian_smoothing_3d(torch.from_numpy(cases.field_mask()).cuda(), cases.FIELD_SIGMA).cpu().numpy()
    assert field.dtype == np.float32 and np.isfinite(field).all() and field.max() > 0.5
    rec["field_a"] = field
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
