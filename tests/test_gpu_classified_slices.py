"""GPU: the classifier filter inside the device-resident slice pipeline, on bit-packed masks from the mask generator to the painted plane.

  * Predictor.predict_bits / batch_predict_bits against predict / batch_predict on the unpacked stack: np.array_equal.  The two routes
    share every kernel after the crop, the crop kernel's image arithmetic is one template body, and predict is bit-repeatable
    (tests/test_gpu_classifier.py), so the probabilities, the image crops, the mask crops and their areas are the same bits.
  * Engine.consensus_components_bits against consensus_components on the same stack: label plane and the integer columns exact; the
    score of either within the any-order fp64 summation bound of the exact per-component mean (formula below).
  * Engine.relabel_plane against numpy.
  * The slice chain (consensus on bits -> paint table -> relabel) against the host convert_predictions_to_masks + paint loop.
  * propagationSegmenter.slice_by_slice_device with a classifier against slice_by_slice, with two handles in flight.

Score bound: avg (the per-pixel overlap-averaged confidence) is recomputed in numpy as the host code computes it (float32 chain in list
order, float64 division); with exact = fsum(avg[comp]) / area and u = 2^-53 a score must satisfy
|score - exact| <= (area u / (1 - area u)) fsum(|avg[comp]|) / area."""
import math
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import classified_slice_ref as ref
from saber_amd.utils import npz_parts

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
G = npz_parts.load(ref.GOLDEN)
NC = 3


def dev_bits(stack_bool, garbage_past_w=False):
    """the packed stack on the device as amg_generate returns it (int32); garbage_past_w also sets every bit past W in the rows' last
    words, which the C-ABI says are ignored"""
    bits = ref.pack_bits(stack_bool)
    W = stack_bool.shape[2]
    if garbage_past_w and W % 32:
        bits = bits.copy()
        bits[..., -1] |= np.uint32((0xFFFFFFFF << (W % 32)) & 0xFFFFFFFF)
    return torch.from_numpy(bits.view(np.int32)).cuda()


def u16(t):
    """a uint16 device plane as a numpy array (through the int16 view, which every torch build copies)"""
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def setup():
    from oracle import classifier_ref as cr
    from saber_amd.classifier.models.predictor import Predictor
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import seeded_weights
    cfg = get_config("tiny")
    eng = Engine("tiny", weights=seeded_weights(cfg, 0), max_images=4, max_prompts=64)
    config = {"model": {"num_classes": NC}, "amg_params": {"sam2_cfg": "tiny"}}
    pred = Predictor(None, None, config=config, head_weights=cr.seeded_head(NC, 0), engine=eng)
    return eng, pred


# ---------------------------------------------------------------------------------------------- 1. classifier on bit-packed rows
def test_batch_predict_bits_equals_batch_predict_on_the_golden_masks(setup):
    eng, pred = setup
    masks = G["masks"]
    assert masks.shape == (8, 200, 240) and sorted((masks > 0).sum(axis=(1, 2)).tolist())[:3] == [0, 1, 31]
    bits = dev_bits(masks > 0)
    rows = [5, 0, 7, 3, 1, 2, 6, 4]
    want = pred.batch_predict(G["image"], masks[rows], batch_size=3)
    got = pred.batch_predict_bits(G["image"], bits, rows, 240, batch_size=3)
    assert got.shape == (8, NC) and got.dtype == np.float32
    assert np.array_equal(got, want)
    assert (want.sum(axis=1) > 0).sum() == 7 and np.all(want[rows.index(6)] == 0)      # the empty mask is filtered, the others classified


def test_predict_bits_crops_equal_predict_crops(setup):
    eng, pred = setup
    masks = G["masks"]
    rows = [5, 0, 7, 3, 1, 2, 6, 4]
    p_u8 = pred.predict(G["image"], masks[rows])
    crops_u8, cm_u8 = (t.cpu().numpy() for t in pred.last_crops(8))
    p_bits = pred.predict_bits(G["image"], dev_bits(masks > 0), rows, 240)
    crops_b, cm_b = (t.cpu().numpy() for t in pred.last_crops(8))
    assert np.array_equal(cm_b, cm_u8)
    assert np.array_equal(cm_b.sum(axis=(1, 2), dtype=np.int64), G["crops_mask_area"][rows])
    assert np.array_equal(crops_b, crops_u8)
    assert np.array_equal(p_bits, p_u8)


def _small_case(name):
    rng = np.random.default_rng(len(name))
    if name == "w20":                              # a single, partial word per row
        H, W = 30, 20
        st = np.zeros((4, H, W), dtype=bool)
        st[0, 4:20, 3:15] = True
        st[1, 11, 19] = True                       # the image's last column
        st[2] = True
        st[3, 0:9, 0:2] = True
    elif name == "w64":                            # two full words: the bits on either side of the word boundary and at both ends
        H, W = 16, 64
        st = np.zeros((4, H, W), dtype=bool)
        st[0, 3, [0, 31, 32, 63]] = True
        st[1, 5:9, 31:33] = True
        st[2, 2:14, 63] = True
        st[3, 7, 0] = True
    else:
        raise KeyError(name)
    return rng.normal(100.0, 20.0, (H, W)).astype(np.float32), st


@pytest.mark.parametrize("name", ["w20", "w64"])
def test_predict_bits_at_word_edges(setup, name):
    eng, pred = setup
    image, st = _small_case(name)
    n, W = st.shape[0], st.shape[2]
    want = pred.predict(image, st.astype(np.uint8))
    crops_u8, cm_u8 = (t.cpu().numpy() for t in pred.last_crops(n))
    got = pred.predict_bits(image, dev_bits(st, garbage_past_w=True), list(range(n)), W)
    crops_b, cm_b = (t.cpu().numpy() for t in pred.last_crops(n))
    assert np.array_equal(cm_b, cm_u8) and np.array_equal(crops_b, crops_u8)
    assert np.array_equal(got, want) and (want.sum(axis=1) > 0).all()


def test_predict_bits_argument_errors(setup):
    eng, pred = setup
    bits = dev_bits(G["masks"] > 0)
    assert pred.predict_bits(G["image"], bits, [], 240).shape == (0, NC)
    with pytest.raises(ValueError):
        pred.predict_bits(G["image"], bits, [8], 240)                      # row outside the stack
    with pytest.raises(ValueError):
        pred.predict_bits(G["image"], bits, [0], 256)                      # W does not match the image
    with pytest.raises(ValueError):
        pred.predict_bits(G["image"], bits.cpu(), [0], 240)


# ---------------------------------------------------------------------------------------------- 2. consensus on bit-packed rows
def _discs(rng, h, w, n, rmin, rmax):
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((n, h, w), dtype=bool)
    for i in range(n):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(rmin, rmax + 1)
        out[i] = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return out


def consensus_scene(name):
    """-> (stack bool (n,H,W), select)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    sel = None
    if name == "discs_37x67":
        st = _discs(rng, 37, 67, 9, 3, 9)
    elif name == "deep_37x67":
        st = np.zeros((12, 37, 67), dtype=bool)
        for i in range(12):
            y0, x0 = rng.integers(0, 12), rng.integers(0, 20)
            st[i, y0:y0 + rng.integers(15, 25), x0:x0 + rng.integers(30, 47)] = True
        assert st.sum(0).max() >= 8
    elif name == "bars_5x130":
        st = np.zeros((4, 5, 130), dtype=bool)
        st[0, 1, 3:129] = True
        st[1, 0:3, 60:70] = True
        st[2, 4, :] = True
        st[3, 3, 64] = True
    elif name == "seams_7x600":                   # runs across, up to and from the 256-pixel seams and the 32-bit word boundaries
        st = np.zeros((5, 7, 600), dtype=bool)
        st[0, 0, 20:40] = True                    # across columns 31/32
        st[0, 1, 31] = True                       # ends on a word's last bit ...
        st[1, 1, 32] = True                       # ... where another mask's first bit continues the run
        st[1, 2, 250:260] = True                  # across 255/256
        st[2, 3, 200:256] = True                  # ends at the seam ...
        st[3, 3, 256:300] = True                  # ... where another mask begins
        st[2, 4, 505:520] = True                  # across 511/512
        st[3, 5, 511] = True
        st[4, 5, 512:] = True
        st[4, 6, :] = True                        # a whole row
        st[0, 6, 100:400] = True                  # ... partly under a second mask: the average changes at 255/256 inside one run
    elif name == "one_pixel":
        st = np.ones((1, 1, 1), dtype=bool)
    elif name == "alternating_1x200":
        st = np.zeros((2, 1, 200), dtype=bool)
        st[0, 0, ::2] = True
        st[1, 0, ::4] = True
    elif name == "skip_and_permute":
        st = _discs(rng, 41, 70, 9, 4, 12)
        sel = [7, 2, 5, 0]
    else:
        raise KeyError(name)
    k = st.shape[0] if sel is None else len(sel)
    conf = rng.uniform(0.34, 1.0, k).astype(np.float32)
    return st, conf, list(range(st.shape[0])) if sel is None else sel


def host_avg(st, rows, conf):
    """count and avg as filters/masks.py::_consensus_based_resolution computes them"""
    cm = np.zeros(st.shape[1:], dtype=np.float32)
    count = np.zeros(st.shape[1:], dtype=np.int32)
    for r, c in zip(rows, conf):
        cm += st[r] * c
        count += st[r]
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.nan_to_num(np.divide(cm, count))
    assert cm.dtype == np.float32 and avg.dtype == np.float64
    return count, avg


def assert_scores(scores, labels, avg, what):
    for i, score in enumerate(scores):
        vals = avg[labels == i + 1]
        area = int(vals.size)
        exact = math.fsum(vals) / area
        bound = (area * U / (1.0 - area * U)) * math.fsum(np.abs(vals)) / area
        assert abs(float(score) - exact) <= bound, f"{what}: component {i} (area {area}): |score - exact| = {abs(float(score) - exact):.3e} > {bound:.3e}"


@pytest.mark.parametrize("name", ["discs_37x67", "deep_37x67", "bars_5x130", "seams_7x600", "one_pixel", "alternating_1x200", "skip_and_permute"])
def test_consensus_bits_equals_consensus_on_the_uint8_stack(setup, name):
    eng, _ = setup
    st, conf, rows = consensus_scene(name)
    W = st.shape[2]
    l_u8, t_u8 = eng.consensus_components(torch.from_numpy(st.astype(np.uint8)).cuda(), rows, conf)
    l_b, t_b = eng.consensus_components_bits(dev_bits(st, garbage_past_w=True), W, rows, conf)
    assert l_b.dtype == torch.int32 and tuple(l_b.shape) == st.shape[1:] and l_b.is_cuda
    count, avg = host_avg(st, rows, conf)
    want, ncomp = ndimage.label(count > 0)
    labels = l_b.cpu().numpy()
    assert np.array_equal(labels, want.astype(np.int32)) and torch.equal(l_b, l_u8)
    assert t_b["area"].size == ncomp > 0
    for key in ("area", "x_min", "y_min", "x_max", "y_max"):
        assert t_b[key].tolist() == t_u8[key].tolist(), key
    assert t_b["area"].tolist() == np.bincount(want.ravel())[1:].tolist()
    assert_scores(t_b["score"], want, avg, "bit-packed route")
    assert_scores(t_u8["score"], want, avg, "uint8 route")
    if name == "deep_37x67":
        assert count.max() >= 8 and np.unique(conf).size == conf.size
    if name == "seams_7x600":
        assert ncomp == 3 and count.max() == 2
    if name == "alternating_1x200":
        assert ncomp == 100


def test_consensus_bits_capacity_protocol_and_errors(setup):
    eng, _ = setup
    st, conf, rows = consensus_scene("alternating_1x200")
    bits = dev_bits(st)
    l0, t0 = eng.consensus_components_bits(bits, 200, rows, conf)
    l1, t1 = eng.consensus_components_bits(bits, 200, rows, conf, capacity=1)
    assert torch.equal(l0, l1) and t0["area"].tolist() == t1["area"].tolist() and t1["area"].size == 100
    with pytest.raises(ValueError):
        eng.consensus_components_bits(bits, 200, [2], conf[:1])            # row outside the stack
    with pytest.raises(ValueError):
        eng.consensus_components_bits(bits, 300, rows, conf)               # W does not match the words per row
    with pytest.raises(ValueError):
        eng.consensus_components_bits(bits, 200, [], conf[:0])


# ---------------------------------------------------------------------------------------------- 3. paint by table
@pytest.mark.parametrize("shape", [(37, 67), (7, 600)])
def test_relabel_plane_equals_numpy(setup, shape):
    eng, _ = setup
    rng = np.random.default_rng(shape[1])
    K = 23
    labels = rng.integers(0, K + 1, shape).astype(np.int32)
    lut = rng.permutation(K + 1).astype(np.uint16) * 2500          # values past 32767: the plane is unsigned
    lut[0] = 0
    lut[[3, 9, 17]] = 0
    plane = eng.relabel_plane(torch.from_numpy(labels).cuda(), lut)
    assert plane.dtype == torch.uint16 and tuple(plane.shape) == shape
    assert np.array_equal(u16(plane), lut[labels])
    assert lut.max() > 32767 and (lut[labels] == 0).any()


# ---------------------------------------------------------------------------------------------- 4. the slice chain on the golden masks
@pytest.mark.parametrize("target", [1, 2])
def test_slice_chain_equals_host_filter_and_paint(setup, target):
    from saber_amd.filters import masks as fm
    from saber_amd.segmenters.slice_driver import classified_paint_lut
    eng, _ = setup
    st, probs = G["masks"] > 0, ref.golden_predictions()
    want, n_want = ref.host_plane(fm, st, probs, target, 32)
    keep = [j for j, p in enumerate(probs.argmax(1)) if p == target]
    labels, table = eng.consensus_components_bits(dev_bits(st), 240, keep, probs[keep, target])
    lut = classified_paint_lut(table["area"], 32)
    plane = u16(eng.relabel_plane(labels, lut))
    assert np.array_equal(plane, want)
    assert plane.max() == n_want == int(np.count_nonzero(lut)) >= 1


# ---------------------------------------------------------------------------------------------- 5. end to end, 6. guards
def _volume(Z=3, S=384):
    rng = np.random.default_rng(11)
    vol = rng.normal(32768, 3000, (Z, S, S))
    zz, yy, xx = np.mgrid[:Z, :S, :S]
    for _ in range(9):
        cy, cx, r = rng.integers(40, S - 40, 2).tolist() + [int(rng.integers(15, 60))]
        vol[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += rng.choice([-6000, 6000])
    return np.clip(vol, 0, 65535).astype(np.float32)


def _head(favoured):
    """a seeded 3-class head whose last bias favours one class by 10: every mask that passes the crop-area filter gets that class"""
    from oracle import classifier_ref as cr
    Wh = {k: v.copy() for k, v in cr.seeded_head(NC, 0).items()}
    Wh["classifier.4.bias"][favoured] += 10.0
    return Wh


@pytest.fixture(scope="module")
def classified():
    os.environ["SABER_AMD_SEEDED_WEIGHTS"] = "1"               # no checkpoint offline: deterministic synthetic weights
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.amg import cfgAMG
    from saber_amd.adapters.sam2.automask import get_engine
    from saber_amd.classifier.models.predictor import Predictor
    from saber_amd.segmenters.propagation import propagationSegmenter
    amg = cfgAMG(npoints=8, crop_n_layers=1, pred_iou_thresh=0.2, stability_score_thresh=0.3, sam2_cfg="small")
    eng = get_engine("small", "cuda:0")
    config = {"model": {"num_classes": NC}, "amg_params": {"sam2_cfg": "small"}}
    pred = Predictor(None, None, config=config, head_weights=_head(1), engine=eng, min_area=50)
    nobody = Predictor(None, None, config=config, head_weights=_head(0), engine=eng, min_area=50)
    seg = propagationSegmenter(deviceID=0, cfg=SAM2AdapterConfig(cfg="tiny", amg_cfg=amg, classifier=pred, min_mask_area=50), min_mask_area=50)
    return seg, pred, nobody, _volume()


def test_slice_loop_with_classifier_device_equals_host(classified):
    from saber_amd.adapters.sam2.automask import get_replica
    seg, pred, _, vol = classified
    assert seg.classifier is pred and seg.batchsize == 32
    ref_vol = seg.slice_by_slice(vol)                              # host dict route: classifier, scipy consensus, numpy paint, host 3-D CC
    dev_vol = seg.slice_by_slice_device(vol)                       # two handles in flight, everything on bit-packed rows
    assert ref_vol.dtype == np.uint32 and dev_vol.dtype == np.uint32 and ref_vol.shape == vol.shape
    assert ref_vol.max() > 0, "no component survived: the test volume / thresholds no longer exercise the path"
    assert np.array_equal(ref_vol, dev_vol)
    # the planes, against the host loop's planes
    planes = seg.slice_by_slice_device(vol, stitch=False)
    host_planes = np.zeros(vol.shape, dtype=np.uint16)
    for z in range(vol.shape[0]):
        for idx, m in enumerate(seg.segment_image(vol[z], display=False)):
            host_planes[z][m["segmentation"]] = idx + 1
    assert planes.dtype == np.uint16 and np.array_equal(planes, host_planes) and host_planes.max() > 0
    # the classifier is looked at: the same segmenter without it paints something else
    seg.classifier = None
    try:
        unfiltered = seg.slice_by_slice_device(vol, stitch=False)
    finally:
        seg.classifier = pred
    assert not np.array_equal(planes, unfiltered)
    # thread 1 ran a replica of the classifier on the second handle of the classifier's model
    second = get_replica(pred.engine, 1)
    rep = pred.replica(second)
    assert rep is not pred and rep.engine is second and second is not pred.engine and second.cfg.name == "small"
    assert rep in pred._replicas.values() and pred.replica(second) is rep and pred.replica(pred.engine) is pred
    assert rep.min_area == pred.min_area and rep.num_classes == NC


def test_slice_guards(classified):
    from saber_amd.segmenters.slice_driver import segment_slice_to_plane
    seg, pred, nobody, vol = classified
    gen = seg.adapter._generator()
    eng, params = gen.base_generator.engine, gen.base_generator.params
    sl = torch.from_numpy(vol[0]).to(eng.device)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="target_class"):
            segment_slice_to_plane(eng, sl, params, min_mask_area=50, classifier=pred, target_class=bad)
    plane, n = segment_slice_to_plane(eng, sl, params, min_mask_area=50, classifier=pred, target_class=1, classifier_min_area=32)
    assert n > 0 and int(u16(plane).max()) == n
    # a head that calls everything class 0: nothing of the target class
    plane, n = segment_slice_to_plane(eng, sl, params, min_mask_area=50, classifier=nobody, target_class=1, classifier_min_area=32)
    assert n == 0 and plane.dtype == torch.uint16 and tuple(plane.shape) == vol.shape[1:] and not u16(plane).any()
