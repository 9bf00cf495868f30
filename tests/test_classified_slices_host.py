"""CPU: the host decisions of the classified slice route (saber_amd.segmenters.slice_driver): the paint table built from the consensus
component areas, and the route's selection + paint restated on the host against filters.masks.convert_predictions_to_masks with scipy."""
import numpy as np
import pytest

import classified_slice_ref as ref
from saber_amd.utils import npz_parts


def lut_of(areas, min_area):
    from saber_amd.segmenters.slice_driver import classified_paint_lut
    return classified_paint_lut(areas, min_area)


def test_lut_ranks_by_ascending_area():
    lut = lut_of([500, 40, 900, 41], 32)
    assert lut.dtype == np.uint16 and lut.tolist() == [0, 3, 1, 4, 2]


def test_lut_ties_keep_label_order():
    assert lut_of([70, 50, 70, 50, 70], 0).tolist() == [0, 3, 1, 4, 2, 5]


def test_lut_threshold_is_inclusive_and_the_rest_is_zero():
    assert lut_of([31, 32, 33, 5, 32], 32).tolist() == [0, 0, 1, 3, 0, 2]
    assert lut_of([31, 5], 32).tolist() == [0, 0, 0]


def test_lut_of_an_empty_table():
    lut = lut_of([], 32)
    assert lut.dtype == np.uint16 and lut.tolist() == [0]
    assert lut_of(np.zeros(0, dtype=np.int64), 0).tolist() == [0]


def test_lut_overflow_raises():
    assert int(lut_of(np.full(65535, 40), 32).max()) == 65535
    with pytest.raises(ValueError, match="65535"):
        lut_of(np.full(65536, 40), 32)
    assert lut_of(np.concatenate([np.full(65535, 40), np.full(10, 3)]), 32).size == 65546      # the small ones do not count


def _scene():
    """14 discs and 5 sprinkles of single pixels in a 90x131 image; classes dealt so that 1 and 2 each hold overlapping discs"""
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[:90, :131]
    st = np.zeros((19, 90, 131), dtype=bool)
    for i in range(14):
        cy, cx, r = rng.integers(0, 90), rng.integers(0, 131), rng.integers(2, 15)
        if i in (4, 5):                            # same class as disc i - 3 (classes go round by i % 3): an overlapping pair in 1 and in 2
            cy, cx, r = 30 + 25 * (i - 4), 40 + 50 * (i - 4), 9
            st[i - 3] = (yy - cy) ** 2 + (xx - cx - 6) ** 2 <= 49
        st[i] = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    st[14:] = rng.random((5, 90, 131)) < 0.002
    cls = np.arange(19) % 3
    conf = rng.uniform(0.5, 0.95, 19).astype(np.float32)
    probs = np.full((19, 3), 0.0, dtype=np.float32)
    for i in range(19):
        probs[i] = (1.0 - conf[i]) / 2
        probs[i, cls[i]] = conf[i]
    return st, probs


@pytest.mark.parametrize("min_area", [0, 32, 40])
@pytest.mark.parametrize("target", [1, 2])
def test_restated_route_equals_convert_predictions_to_masks(target, min_area):
    from saber_amd.filters import masks as fm
    st, probs = _scene()
    own = [i for i in range(len(st)) if probs[i].argmax() == target]
    assert len(own) >= 2 and any((st[a] & st[b]).any() for a in own for b in own if a < b), "no overlapping pair in the class"
    want, n_want = ref.host_plane(fm, st, probs, target, min_area)
    got, n_got = ref.restated_plane(st, probs, target, min_area)
    assert got.dtype == np.uint16 and n_got == n_want > 0
    assert np.array_equal(got, want)
    if min_area == 40:
        assert n_want < ref.host_plane(fm, st, probs, target, 0)[1]           # the filter removed something


@pytest.mark.parametrize("target", [1, 2])
def test_restated_route_on_the_golden_masks(target):
    from saber_amd.filters import masks as fm
    G = npz_parts.load(ref.GOLDEN)
    st, probs = G["masks"] > 0, ref.golden_predictions()
    want, n_want = ref.host_plane(fm, st, probs, target, 32)
    got, n_got = ref.restated_plane(st, probs, target, 32)
    assert np.array_equal(got, want) and n_got == n_want == {1: 1, 2: 2}[target]
    assert want.max() == n_want


def test_nobody_of_the_target_class_gives_a_zero_plane():
    st, probs = _scene()
    probs = probs.copy()
    probs[:, 0] = 2.0
    got, n = ref.restated_plane(st, probs, 1, 0)
    assert n == 0 and not got.any()


def test_pack_bits_layout():
    st = np.zeros((1, 2, 40), dtype=bool)
    st[0, 1, 33] = st[0, 0, 0] = st[0, 0, 31] = True
    bits = ref.pack_bits(st)
    assert bits.shape == (1, 2, 2) and bits.dtype == np.uint32
    assert bits[0, 1].tolist() == [0, 2] and bits[0, 0].tolist() == [1 | (1 << 31), 0]
