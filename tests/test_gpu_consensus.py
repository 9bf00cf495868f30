"""GPU: csrc/consensus2d.hip (overlap-averaged confidence, 4-connected 2-D components, per-component table) and the opt-in device route
of saber_amd.filters.masks on top of it.  The yardstick is the unchanged host route of _consensus_based_resolution (the line-for-line
restatement of saber/filters/masks.py:64-121, with scipy): component count, order, every segmentation, area, bbox, point_coords and
crop_box by exact equality, the label plane against scipy.ndimage.label(count > 0) by exact equality.

Score bound: avg (the per-pixel overlap-averaged confidence) is recomputed in numpy as the host code computes it; with
exact = fsum(avg[comp]) / area and u = 2^-53 a score must satisfy |score - exact| <= (area u / (1 - area u)) fsum(|avg[comp]|) / area: the
any-order bound of an fp64 summation of `area` terms plus one division.  It assumes avg bit-equal to the reference's: a float32
accumulation in another order is off by ~2^-24, seven orders of magnitude above it (case "deep": up to 12 masks per pixel with distinct
random float32 confidences).  The host route's own score is held to the same bound, so the bound is checked against the yardstick."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    from saber_amd.filters._context import handle
    return handle(0)


@pytest.fixture(scope="module")
def fm():
    from saber_amd.filters import masks
    return masks


# ---------------------------------------------------------------------------------------------- scenes: (stack bool (n,H,W), conf float32 (k,), select or None)
def _conf(rng, k):
    return rng.uniform(0.34, 1.0, k).astype(np.float32)


def _discs(rng, h, w, n, rmin, rmax):
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((n, h, w), dtype=bool)
    for i in range(n):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(rmin, rmax + 1)
        out[i] = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return out


def _with_partial(pattern, rng):
    """the pattern as one mask plus two partial copies, so that the per-pixel count and average vary inside a component"""
    h, w = pattern.shape
    a, b = pattern.copy(), pattern.copy()
    a[:, : w // 3] = False
    b[h // 2:, :] = False
    return np.stack([pattern, a, b])


def scene(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    sel = None
    if name == "discs_37x67":
        st = _discs(rng, 37, 67, 9, 3, 9)
    elif name == "deep_37x67":                    # rectangles that pile up: pixels under 8 and more masks
        st = np.zeros((12, 37, 67), dtype=bool)
        for i in range(12):
            y0, x0 = rng.integers(0, 12), rng.integers(0, 20)
            st[i, y0:y0 + rng.integers(15, 25), x0:x0 + rng.integers(30, 47)] = True
        assert st.sum(0).max() >= 8
    elif name == "bars_5x130":
        st = np.zeros((4, 5, 130), dtype=bool)
        st[0, 1, 3:129] = True                    # a run across two chunk boundaries
        st[1, 0:3, 60:70] = True
        st[2, 4, :] = True                        # a whole row
        st[3, 3, 64] = True                       # the bridge between rows 1 and 4 sits on a chunk's first pixel
    elif name == "seams_7x600":                  # the kernels cut a row into 256-pixel segments: runs across, up to and from the seams
        st = np.zeros((4, 7, 600), dtype=bool)
        st[0, 0, 100:400] = True
        st[0, 1, 399] = True
        st[0, 2, :] = True
        st[1, 4, 200:256] = True                  # ends at a seam ...
        st[2, 4, 256:300] = True                  # ... where another mask begins
        st[1, 5, 511:513] = True
        st[2, 6, 512:] = True
        st[3, 0:3, 250:520] = True
    elif name == "one_pixel":
        st = np.ones((1, 1, 1), dtype=bool)
    elif name == "alternating_1x200":
        st = np.zeros((2, 1, 200), dtype=bool)
        st[0, 0, ::2] = True
        st[1, 0, ::4] = True
    elif name == "column_64x1":
        st = np.zeros((2, 64, 1), dtype=bool)
        st[0, 3:20, 0] = True
        st[0, 22, 0] = True
        st[1, 40:, 0] = True
    elif name == "checkerboard_32x33":
        yy, xx = np.mgrid[:32, :33]
        st = ((yy + xx) % 2 == 0)[None]
    elif name == "serpentine_48x96":             # arms on the even rows, joined alternately at the right and at the left end
        p = np.zeros((48, 96), dtype=bool)
        p[::2, :] = True
        for j, y in enumerate(range(1, 47, 2)):
            p[y, 95 if j % 2 == 0 else 0] = True
        st = _with_partial(p, rng)
    elif name == "comb_bottom_48x96":            # teeth on the even columns, joined by the last row only
        p = np.zeros((48, 96), dtype=bool)
        p[:, ::2] = True
        p[47, :] = True
        st = _with_partial(p, rng)
    elif name == "comb_right_48x96":             # arms on the even rows, joined by the last column only
        p = np.zeros((48, 96), dtype=bool)
        p[::2, :] = True
        p[:, 95] = True
        st = _with_partial(p, rng)
    elif name == "diagonal_touch":
        st = np.zeros((2, 20, 24), dtype=bool)
        st[0, 2:8, 3:9] = True
        st[1, 8:13, 9:15] = True                  # corner to corner with the first
        st[1, 1:2, 9:12] = True                   # and a corner contact from above
    elif name == "borders_30x70":
        st = np.zeros((5, 30, 70), dtype=bool)
        st[0, 0, 5:60] = True
        st[1, 29, 10:70] = True
        st[2, 5:25, 0] = True
        st[3, 3:27, 69] = True
        st[4, 0, 0] = st[4, 0, 69] = st[4, 29, 0] = True
    elif name == "full_40x150":
        st = np.zeros((3, 40, 150), dtype=bool)
        st[0] = True
        st[1, 5:30, 20:140] = True
        st[2, :, 100:] = True
    elif name == "random_37x67":
        st = rng.random((40, 37, 67)) < 0.008
    elif name == "single_mask":
        st = _discs(rng, 37, 67, 1, 6, 10)
    elif name == "permuted_subset":
        st = _discs(rng, 41, 70, 9, 4, 12)
        sel = [7, 2, 5, 0]
    elif name == "repeated_empty":
        st = _discs(rng, 41, 70, 6, 4, 12)
        st[4] = False
        sel = [3, 4, 1, 4]
    elif name == "discs_1024":
        st = _discs(rng, 1024, 1024, 30, 20, 110)
    else:
        raise KeyError(name)
    k = st.shape[0] if sel is None else len(sel)
    return st, _conf(rng, k), sel


SCENES = ["discs_37x67", "deep_37x67", "bars_5x130", "seams_7x600", "one_pixel", "alternating_1x200", "column_64x1", "checkerboard_32x33", "serpentine_48x96",
          "comb_bottom_48x96", "comb_right_48x96", "diagonal_touch", "borders_30x70", "full_40x150", "random_37x67", "single_mask",
          "permuted_subset", "repeated_empty", "discs_1024"]
EXPECTED_COMPONENTS = {"seams_7x600": 3, "one_pixel": 1, "alternating_1x200": 100, "column_64x1": 3, "checkerboard_32x33": 528, "serpentine_48x96": 1,
                       "comb_bottom_48x96": 1, "comb_right_48x96": 1, "diagonal_touch": 3, "borders_30x70": 7, "full_40x150": 1}


# ---------------------------------------------------------------------------------------------- comparisons
def host_avg(shape, masks, conf):
    """count and avg as the host code computes them (filters/masks.py, _consensus_based_resolution)"""
    cm = np.zeros(shape, dtype=np.float32)
    count = np.zeros(shape, dtype=np.int32)
    for m, c in zip(masks, conf):
        cm += m["segmentation"] * c
        count += m["segmentation"]
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.nan_to_num(np.divide(cm, count))
    assert cm.dtype == np.float32 and avg.dtype == np.float64
    return count, avg


def assert_same_lists(dev, host):
    assert len(dev) == len(host)
    for i, (d, h) in enumerate(zip(dev, host)):
        assert list(d) == list(h), f"component {i}: keys"
        assert d["segmentation"].dtype == np.bool_ and d["segmentation"].shape == h["segmentation"].shape
        assert np.array_equal(d["segmentation"], h["segmentation"]), f"component {i}: segmentation"
        for key in ("area", "bbox", "point_coords", "crop_box"):
            assert d[key] == h[key], f"component {i}: {key} {d[key]} != {h[key]}"
        assert type(d["area"]) is int and all(type(v) is int for v in d["bbox"] + d["crop_box"] + d["point_coords"][0])
        assert type(d["predicted_iou"]) is float
        assert d["predicted_iou"] == d["stability_score"] and h["predicted_iou"] == h["stability_score"]


def assert_scores(found, avg, what):
    """the any-order fp64 summation bound of the module docstring, for every component of a dict list"""
    worst = 0.0
    for i, m in enumerate(found):
        vals = avg[m["segmentation"]]
        area = int(vals.size)
        exact = math.fsum(vals) / area
        bound = (area * U / (1.0 - area * U)) * math.fsum(np.abs(vals)) / area
        err = abs(m["predicted_iou"] - exact)
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
        assert err <= bound, f"{what}: component {i} (area {area}): |score - exact| = {err:.3e} > {bound:.3e}"
    return worst


def run_case(ctx, fm, st, conf, sel, via_stack):
    h, w = st.shape[1:]
    rows = list(range(st.shape[0])) if sel is None else sel
    masks = [{"segmentation": st[i]} for i in rows]
    host = fm._consensus_based_resolution((h, w), masks, conf)
    stack_dev = torch.from_numpy(st.astype(np.uint8)).cuda()
    if via_stack:
        dev = fm._consensus_based_resolution((h, w), masks, conf, device=0, masks_dev=stack_dev, select=rows)
    else:
        dev = fm._consensus_based_resolution((h, w), masks, conf, device=0)
    assert_same_lists(dev, host)
    count, avg = host_avg((h, w), masks, conf)
    labels, table = ctx.consensus_components(stack_dev, rows, conf)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (h, w) and labels.is_cuda
    want, ncomp = ndimage.label(count > 0)
    assert np.array_equal(labels.cpu().numpy(), want.astype(np.int32))
    assert table["area"].size == ncomp == len(host)
    assert table["area"].tolist() == [m["area"] for m in host]
    r_host = assert_scores(host, avg, "host route")
    r_dev = assert_scores(dev, avg, "device route")
    print(f"components {ncomp}, max count {int(count.max())}, worst |score - exact| / bound: host {r_host:.3f}, device {r_dev:.3f}")
    return dev, host, count


@pytest.mark.parametrize("name", SCENES)
def test_device_route_equals_host_route(ctx, fm, name):
    st, conf, sel = scene(name)
    dev, host, count = run_case(ctx, fm, st, conf, sel, via_stack=sel is not None)
    if name in EXPECTED_COMPONENTS:
        assert len(dev) == EXPECTED_COMPONENTS[name]
    if name == "random_37x67":
        assert len(dev) > 200
    if name == "deep_37x67":
        assert count.max() >= 8 and np.unique(conf).size == conf.size
    if name == "discs_1024":
        assert 2 <= len(dev) <= 30


def test_upload_and_resident_stack_agree(ctx, fm):
    st, conf, _ = scene("discs_37x67")
    a, _, _ = run_case(ctx, fm, st, conf, None, via_stack=False)
    b, _, _ = run_case(ctx, fm, st, conf, None, via_stack=True)
    assert_same_lists(a, b)


def test_all_empty_selection_gives_an_empty_list(ctx, fm):
    st = np.zeros((3, 20, 70), dtype=bool)
    conf = np.array([0.5, 0.6, 0.7], dtype=np.float32)
    masks = [{"segmentation": m} for m in st]
    assert fm._consensus_based_resolution((20, 70), masks, conf) == []
    assert fm._consensus_based_resolution((20, 70), masks, conf, device=0) == []
    assert fm._consensus_based_resolution((20, 70), [], conf[:0], device=0) == []
    labels, table = ctx.consensus_components(torch.from_numpy(st.astype(np.uint8)).cuda(), [0, 1, 2], conf)
    assert int(labels.abs().sum()) == 0 and table["area"].size == 0 and table["score"].size == 0


def test_float64_confidences_are_cast_to_float32(ctx, fm):
    st, conf, _ = scene("deep_37x67")
    rng = np.random.default_rng(5)
    conf64 = rng.uniform(0.34, 1.0, conf.size)
    masks = [{"segmentation": m} for m in st]
    a = fm._consensus_based_resolution((37, 67), masks, conf64, device=0)
    b = fm._consensus_based_resolution((37, 67), masks, conf64.astype(np.float32), device=0)
    assert_same_lists(a, b)
    _, avg = host_avg((37, 67), masks, conf64.astype(np.float32))
    assert_scores(a, avg, "float64 confidences")


def test_min_area_drops_components_before_their_arrays(ctx, fm):
    st, conf, _ = scene("random_37x67")
    masks = [{"segmentation": m} for m in st]
    everything = fm._consensus_based_resolution((37, 67), masks, conf)
    want = [m for m in everything if m["area"] >= 3]
    assert 0 < len(want) < len(everything)
    assert_same_lists(fm._consensus_based_resolution((37, 67), masks, conf, device=0, min_area=3), want)
    assert_same_lists(fm._consensus_based_resolution((37, 67), masks, conf, min_area=3), want)


def test_two_calls_give_the_same_integers(ctx):
    st, conf, _ = scene("discs_1024")
    stack = torch.from_numpy(st.astype(np.uint8)).cuda()
    l0, t0 = ctx.consensus_components(stack, range(30), conf)
    l1, t1 = ctx.consensus_components(stack, range(30), conf)
    assert torch.equal(l0, l1)
    for key in ("area", "x_min", "y_min", "x_max", "y_max"):
        assert t0[key].tolist() == t1[key].tolist()
    assert np.allclose(t0["score"], t1["score"], rtol=1e-12, atol=0)


def test_capacity_guess_is_repeated_once(ctx):
    st, conf, _ = scene("random_37x67")
    stack = torch.from_numpy(st.astype(np.uint8)).cuda()
    l0, t0 = ctx.consensus_components(stack, range(40), conf)
    l1, t1 = ctx.consensus_components(stack, range(40), conf, capacity=1)
    assert torch.equal(l0, l1) and t0["area"].size > 200
    for key in ("area", "x_min", "y_min", "x_max", "y_max"):
        assert t0[key].tolist() == t1[key].tolist()


def test_argument_errors_launch_nothing(ctx):
    stack = torch.zeros((3, 8, 9), dtype=torch.uint8, device="cuda")
    conf = np.array([0.5], dtype=np.float32)
    with pytest.raises(ValueError):
        ctx.consensus_components(stack, [], conf[:0])                       # k = 0
    with pytest.raises(ValueError):
        ctx.consensus_components(stack, [3], conf)                          # index out of range
    with pytest.raises(ValueError):
        ctx.consensus_components(stack, [-1], conf)
    with pytest.raises(ValueError):
        ctx.consensus_components(stack, [0, 1, 2, 0], np.ones(4, np.float32))   # k > n
    with pytest.raises(ValueError):
        ctx.consensus_components(stack, [0, 1], conf)                       # one confidence for two masks
    with pytest.raises(ValueError):
        ctx.consensus_components(stack.to(torch.int32), [0], conf)          # not uint8
    with pytest.raises(ValueError):
        ctx.consensus_components(stack.cpu(), [0], conf)                    # not on the device
    with pytest.raises(ValueError):
        ctx.consensus_components(stack[0], [0], conf)                       # not a stack
    # the C-ABI's own checks (status -1 before any launch; the pointers are never followed)
    lib = ctx.lib
    sel, cf, n = (C.c_int * 2)(0, 5), (C.c_float * 2)(0.5, 0.5), C.c_int(7)
    p = C.c_void_p(stack.data_ptr())
    call = lib.saber_consensus_components
    assert call(ctx.h, p, 3, 8, 9, sel, cf, 0, 4, p, p, C.byref(n), None) == -1 and n.value == 0        # k = 0
    assert call(ctx.h, p, 3, 8, 9, sel, cf, 2, 4, p, p, C.byref(n), None) == -1                          # index 5 of 3
    assert b"index 5" in lib.saber_last_error(ctx.h)
    assert call(ctx.h, p, 1, 8, 9, sel, cf, 2, 4, p, p, C.byref(n), None) == -1                          # k > n
    assert call(ctx.h, p, 3, 0, 9, sel, cf, 1, 4, p, p, C.byref(n), None) == -1                          # H = 0
    assert call(ctx.h, p, 3, 8, 0, sel, cf, 1, 4, p, p, C.byref(n), None) == -1                          # W = 0
    assert call(ctx.h, p, 3, 65536, 32768, sel, cf, 1, 4, p, p, C.byref(n), None) == -1                  # H W = 2^31
    assert b"2^31" in lib.saber_last_error(ctx.h)
    assert call(ctx.h, None, 3, 8, 9, sel, cf, 1, 4, p, p, C.byref(n), None) == -1
    assert call(ctx.h, p, 3, 8, 9, sel, cf, 1, 4, p, None, C.byref(n), None) == -1


# ---------------------------------------------------------------------------------------------- through the public functions
class StubClassifier:
    """batch_predict with fixed float32 probabilities; records what it was handed"""

    def __init__(self, probs):
        self.probs = probs
        self.seen = []

    def batch_predict(self, image, masks, batch_size=32):
        self.seen.append(masks)
        assert int(masks.shape[0]) == self.probs.shape[0]
        return self.probs.copy()


def _classified_scene():
    rng = np.random.default_rng(11)
    st = np.concatenate([_discs(rng, 90, 131, 14, 2, 14), rng.random((6, 90, 131)) < 0.002])
    masks = [{"segmentation": m, "area": int(m.sum())} for m in st]
    p1 = rng.uniform(0.05, 0.95, len(masks)).astype(np.float32)
    probs = np.stack([1.0 - p1, p1], axis=1).astype(np.float32)
    return masks, probs


def test_apply_classifier_device_route(fm):
    masks, probs = _classified_scene()
    image = np.zeros((90, 131), dtype=np.float32)
    unfiltered = fm.apply_classifier(image, list(masks), StubClassifier(probs), desired_class=1, min_mask_area=0)
    for m in (0, 40):
        stub_h, stub_d = StubClassifier(probs), StubClassifier(probs)
        host = fm.apply_classifier(image, list(masks), stub_h, desired_class=1, min_mask_area=m)
        dev = fm.apply_classifier(image, list(masks), stub_d, desired_class=1, min_mask_area=m, device=0)
        assert_same_lists(dev, host)
        assert [d["area"] for d in dev] == sorted(d["area"] for d in dev)
        assert isinstance(stub_h.seen[0], np.ndarray)
        assert isinstance(stub_d.seen[0], torch.Tensor) and stub_d.seen[0].is_cuda and stub_d.seen[0].dtype == torch.uint8
        kept = [i for i in range(len(masks)) if probs[i, 1] > probs[i, 0]]
        _, avg = host_avg((90, 131), [masks[i] for i in kept], probs[kept, 1])
        assert_scores(dev, avg, "apply_classifier device route")
        assert_scores(host, avg, "apply_classifier host route")
    assert 0 < len(dev) < len(unfiltered)                                   # an area of 40 removes some components and keeps some
    with pytest.raises(TypeError):                                          # desired_class=None raises as on the host route
        fm.apply_classifier(image, list(masks), StubClassifier(probs), device=0)
    nobody = np.stack([np.ones(len(masks)), np.zeros(len(masks))], axis=1).astype(np.float32)
    assert fm.apply_classifier(image, list(masks), StubClassifier(nobody), desired_class=1, device=0) == []


def test_saber2d_switch_reaches_the_device_route(fm, monkeypatch):
    from saber_amd.segmenters.base import saber2D
    masks, probs = _classified_scene()
    calls = []
    real = fm._consensus_based_resolution

    def recorder(image_shape, found, confidences, **kw):
        calls.append(kw)
        return real(image_shape, found, confidences, **kw)

    monkeypatch.setattr(fm, "_consensus_based_resolution", recorder)
    seg = saber2D.__new__(saber2D)                                          # no adapter, no weights: only what _apply_classifier reads
    seg.min_mask_area, seg.remove_repeating_masks, seg.classifier, seg.batchsize, seg.target_class = 0, False, StubClassifier(probs), 32, 1
    seg.device = torch.device("cuda:0")
    seg.device_consensus = False
    image = np.zeros((90, 131), dtype=np.float32)
    host = seg._apply_classifier(image, [dict(m) for m in masks])
    assert calls[-1]["device"] is None and calls[-1]["masks_dev"] is None
    seg.device_consensus = True
    dev = seg._apply_classifier(image, [dict(m) for m in masks])
    assert calls[-1]["device"] == torch.device("cuda:0") and calls[-1]["masks_dev"].is_cuda and calls[-1]["min_area"] == 32
    assert_same_lists(dev, host)
    assert len(dev) > 0
