"""GPU: the smoother's bytes, pinned.  tests/golden/smooth_parent_bits.npz holds what Engine.smooth_labels and Engine.gaussian_smoothing_3d
gave on the MI355X at the commit before the whole-volume and the z-chunk route were merged into one pipeline (csrc/smooth3d.hip:
sm_convolve), recorded by tools/record_smooth_bits.py.  Both routes claim one summation order - taps ascending, fma - so they must
reproduce those bytes exactly (np.array_equal), not merely inside the 1e-5 threshold band the oracle tests allow.  The volumes
(tests/smooth_parent_bits_cases.py) are the smallest at which the shared kernels take each of their paths: a box deeper than the z tile
whose own range starts inside it, boxes on both sides of the x and y tile edges, the three element sizes, the dense float field."""
import os

import numpy as np
import pytest
import torch

import sharded_smooth_ref as ref
import smooth_parent_bits_cases as cases
from saber_amd.segmenters import smooth

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "smooth_parent_bits.npz"), allow_pickle=False)
CASES = cases.label_cases()


@pytest.fixture(scope="module")
def ctx():
    from saber_amd.engine import Engine
    e = Engine.bare(0)
    yield e
    e.close()


def to_dev(vol):
    v = np.ascontiguousarray(vol)
    return torch.from_numpy(v.view({1: np.uint8, 2: np.int16, 4: np.int32}[v.dtype.itemsize])).cuda()


def check(ctx, vol, scale, want):
    """the whole-volume route and the chunk route for the splits 1, 2, 3 and Z against the recorded bytes"""
    dev = to_dev(vol)
    Z = vol.shape[0]
    whole, n = ctx.smooth_labels(dev, scale)
    assert n == np.unique(vol[vol != 0]).size
    got = whole.cpu().numpy()
    assert got.dtype == want.dtype == np.uint8 and np.array_equal(got, want), f"whole volume: {int((got != want).sum())} voxels differ"
    for parts in sorted({1, 2, 3, Z}):
        out = smooth.smooth_labels_chunks(ctx, [dev[a:b] for a, b in ref.cuts_of(Z, parts)], scale)
        got = torch.cat(out, 0).cpu().numpy()
        assert np.array_equal(got, want), f"{parts} chunks: {int((got != want).sum())} voxels differ"


@pytest.mark.parametrize("name", sorted(CASES))
def test_label_volumes(ctx, name):
    vol, scale = CASES[name]
    assert G[name].any()
    check(ctx, vol, scale, G[name])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_element_sizes(ctx, dtype):
    """`deep` as uint8, as uint16 (handed over as int16) and as int32: one recording"""
    vol, scale = cases.deep()
    check(ctx, vol.astype(dtype), scale, G["deep"])


def test_float_field(ctx):
    """mode 1 of the pipeline: the box is the volume, every plane is written, the output is the fp32 field itself"""
    got = ctx.gaussian_smoothing_3d(torch.from_numpy(cases.field_mask()).cuda(), cases.FIELD_SIGMA).cpu().numpy()
    want = G["field_a"]
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} values differ, max |diff| {float(np.abs(got - want).max()):.3e}"
