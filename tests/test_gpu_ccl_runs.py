"""GPU: the run-start / carry / unite code of csrc/ccl.h through its three consumers (separate_masks: 26-connected 3-D, components6_3d:
6-connected 3-D, consensus_components[_bits]: 4-connected 2-D) at the widths where that code can go wrong: a row shorter than a wave,
the 64-lane chunk edge and the 256-pixel segment seam of cs_accum from either side, a run carried over more than two chunks.
Integer work against scipy.ndimage.label: every comparison is exact equality with nothing excluded."""
import numpy as np
import pytest
import torch
from scipy import ndimage

WIDTHS = [1, 63, 64, 65, 128, 255, 256, 257, 513]
Z3, H = 2, 3


def _all_but(c):
    def row(w):
        r = np.ones(w, bool)
        r[c:c + 1] = False                  # a column past w is simply dropped
        return r
    return row


def _alternating(w):
    return np.arange(w) % 2 == 0


def _from_60(w):
    return np.arange(w) >= 60


def _last(w):
    return np.arange(w) == w - 1


PATTERNS = [("full", lambda w: np.ones(w, bool)), ("but63", _all_but(63)), ("but64", _all_but(64)), ("but255", _all_but(255)),
            ("but256", _all_but(256)), ("alternating", _alternating), ("from60", _from_60), ("last", _last)]


def volumes(w, rows):
    """(name, (rows, w) bool): every pattern on all rows, then the patterns mixed over the rows (row i holds pattern k + i), so that
    runs in neighbouring rows start at different columns"""
    for name, f in PATTERNS:
        yield name, np.tile(f(w), (rows, 1))
    for k in range(len(PATTERNS)):
        yield f"mixed{k}", np.stack([PATTERNS[(k + i) % len(PATTERNS)][1](w) for i in range(rows)])


def ref_components6(m, mode, min_size):
    """the filter of saber_components6_3d from scipy's labels: mode 0 keeps the components of >= min_size voxels (count: kept), mode 1 the
    largest one, the lowest scipy label on a tie (count: found)"""
    lab, n = ndimage.label(m)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    sizes[0] = 0
    if mode == 0:
        keep = sizes >= max(min_size, 1)
        return keep[lab], int(keep.sum())
    if n == 0:
        return np.zeros(m.shape, bool), 0
    best = int(np.flatnonzero(sizes == sizes.max())[0])
    return lab == best, n


def ref_consensus(plane):
    lab, n = ndimage.label(plane)
    boxes = ndimage.find_objects(lab)
    table = {"area": np.bincount(lab.ravel(), minlength=n + 1)[1:], "y_min": [b[0].start for b in boxes], "y_max": [b[0].stop - 1 for b in boxes],
             "x_min": [b[1].start for b in boxes], "x_max": [b[1].stop - 1 for b in boxes]}
    return lab.astype(np.int32), {k: np.asarray(v, dtype=np.int64) for k, v in table.items()}


def pack_bits(plane):
    """(H,W) bool -> (1,H,ceil(W/32)) int32, bit b of word w = pixel 32 w + b"""
    h, w = plane.shape
    padded = np.zeros((h, (w + 31) // 32 * 32), np.uint8)
    padded[:, :w] = plane
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)[None]


@pytest.mark.parametrize("w", WIDTHS)
def test_expectations_are_self_consistent(w):
    """no GPU: the scipy side alone on every (W, pattern) pair, against the component counts the patterns have by construction"""
    by_construction = {"full": 1, "alternating": (w + 1) // 2, "from60": int(w > 60), "last": 1}
    for c in (63, 64, 255, 256):
        by_construction[f"but{c}"] = 1 if c >= w - 1 else 2      # the hole is past the row or its last column, or it splits the row
    for name, rows in volumes(w, Z3 * H):
        vol = rows.reshape(Z3, H, w)
        n26 = ndimage.label(vol, structure=np.ones((3, 3, 3)))[1]
        ref0, kept0 = ref_components6(vol, 0, 1)
        ref2, kept2 = ref_components6(vol, 0, 2)
        ref1, n6 = ref_components6(vol, 1, 0)
        assert np.array_equal(ref0, vol) and kept0 == n6 >= n26 and kept2 <= kept0
        assert not (ref2 & ~vol).any() and not (ref1 & ~vol).any() and (n6 == 0) == (not ref1.any())
        if n6:                                                   # the largest component; among equals the one whose first voxel comes first
            lab6 = ndimage.label(vol)[0]
            sizes = np.bincount(lab6.ravel())[1:]
            largest = np.isin(lab6, np.flatnonzero(sizes == sizes.max()) + 1)
            assert int(ref1.sum()) == sizes.max() and ref1.ravel().argmax() == largest.ravel().argmax()
        if name in by_construction:
            assert n26 == n6 == by_construction[name], (w, name)
    for name, plane in volumes(w, H):
        lab, t = ref_consensus(plane)
        assert int(t["area"].sum()) == int(plane.sum()) and t["area"].size == int(lab.max())
        assert (t["x_min"] <= t["x_max"]).all() and (t["y_min"] <= t["y_max"]).all()
        assert ((t["x_max"] - t["x_min"] + 1) * (t["y_max"] - t["y_min"] + 1) >= t["area"]).all()
        assert np.array_equal(np.unpackbits(pack_bits(plane).view(np.uint8), axis=-1, bitorder="little")[0, :, :w].astype(bool), plane)
        if name in by_construction:
            assert int(lab.max()) == by_construction[name], (w, name)


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    from saber_amd.filters._context import handle
    return handle(0)


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_separate_masks_26(ctx, w):
    for name, rows in volumes(w, Z3 * H):
        vol = rows.reshape(Z3, H, w)
        want, n_want = ndimage.label(vol, structure=np.ones((3, 3, 3)))
        out, n = ctx.separate_masks(torch.from_numpy(vol.astype(np.int16) * 5).cuda(), min_mask_area=0)
        assert n == n_want, (w, name)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.astype(np.uint32)), (w, name)


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_components6(ctx, w):
    for name, rows in volumes(w, Z3 * H):
        vol = rows.reshape(Z3, H, w)
        d = torch.from_numpy(vol.astype(np.uint8)).cuda()
        for mode, min_size in ((0, 1), (0, 2), (1, 0)):
            want, n_want = ref_components6(vol, mode, min_size)
            got, n = ctx.components6_3d(d, mode, min_size)
            assert n == n_want, (w, name, mode, min_size)
            assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8)), (w, name, mode, min_size)


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_consensus_components_4(ctx, w):
    conf = np.ones(1, np.float32)
    for name, plane in volumes(w, H):
        want, table = ref_consensus(plane)
        stack = torch.from_numpy(plane.astype(np.uint8)[None]).cuda()
        bits = torch.from_numpy(pack_bits(plane)).cuda()
        for entry, (labels, got) in (("bytes", ctx.consensus_components(stack, [0], conf)), ("bits", ctx.consensus_components_bits(bits, w, [0], conf))):
            assert np.array_equal(labels.cpu().numpy(), want), (w, name, entry)
            for key, col in table.items():
                assert np.array_equal(got[key], col), (w, name, entry, key)
