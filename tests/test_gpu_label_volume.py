"""GPU: propagated label volumes on the device (csrc/labelvol.hip, saber_amd/utils/labelvol.py).  The four kernels through the C-ABI
against numpy written out here (every result is integer-exact: comparisons are bit for bit), then the opt-in routes end to end:
SAM2Adapter.segment_volume(device_volume=True) and the segmenters with device_volumes = True against their own host routes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAINT_CHUNK = 64          # labels per launch of the stacked paint (csrc/labelvol.hip LV_PAINT_CHUNK)
LUT_LDS = 8192            # table entries the relabel kernel stages in LDS (LV_LUT_LDS)
COUNTS = (1, 7, 8, 9, 4099)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ck(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()


def dev_u16(a):
    """uint16 values as an int16 device tensor holding the same bits"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda()


def host_u16(t):
    return t.cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------ paint_nearest_stack
def _nearest(out, inn):
    return np.clip(np.floor((np.arange(out) + 0.5) * inn / out).astype(np.int64), 0, inn - 1)


def _paint_ref(logits, labels, thr, plane):
    """the sequential loop: object after object, later ones overwrite"""
    ys, xs = _nearest(plane.shape[0], logits.shape[1]), _nearest(plane.shape[1], logits.shape[2])
    out = plane.copy()
    for lg, lab in zip(logits, labels):
        out = np.where(lg[np.ix_(ys, xs)] > thr, np.uint16(lab), out)
    return out


def _paint_case(n, src, dst, seed):
    rng = np.random.default_rng(seed)
    # an object hits ~16 % of the pixels at thr 1.0 (n <= 3) and 0.6 % at thr 2.5 (the long list, so that untouched pixels remain): objects overlap
    logits = rng.normal(0, 1, (n,) + src).astype(np.float32)
    if n >= 3:
        logits[1] = -1.0                                           # one object with no logit above thr
    if n > 3:
        logits[-1] += 1.5                                          # the object of the second launch covers ~16 % too: it must overwrite the first launch's
    labels = [7, 2, 65535][:n] if n <= 3 else rng.permutation(np.concatenate([[65535, 0], rng.integers(1, 65535, n - 2)])).tolist()
    plane = rng.integers(1000, 2000, dst).astype(np.uint16)        # pre-filled: untouched pixels must survive
    return logits, [int(v) for v in labels], plane


@pytest.mark.parametrize("n", [1, 3, PAINT_CHUNK + 1])
@pytest.mark.parametrize("src,dst", [((16, 16), (37, 53)), ((64, 64), (24, 40))])
def test_paint_nearest_stack(gpu_lib, src, dst, n):
    logits, labels, plane = _paint_case(n, src, dst, 100 + n)
    thr = 1.0 if n <= 3 else 2.5
    ref = _paint_ref(logits, labels, thr, plane)
    assert (ref == plane).any() and (ref != plane).any()           # untouched and painted pixels both exist
    if n > 1:
        ys, xs = _nearest(dst[0], src[0]), _nearest(dst[1], src[1])
        assert ((logits[:, ys][:, :, xs] > thr).sum(0) > 1).any(), "no overlap between objects"
    ld, pd, flag = torch.from_numpy(logits).cuda(), dev_u16(plane), torch.zeros(1, dtype=torch.int32, device="cuda")
    lab = (C.c_int * n)(*labels)
    ck(gpu_lib, gpu_lib.saber_k_paint_nearest_stack(ptr(ld), n, src[0], src[1], lab, thr, ptr(pd), dst[0], dst[1], ptr(flag), None))
    assert np.array_equal(host_u16(pd), ref)
    assert int(flag.item()) == 1
    # bit for bit the n single paints of the existing kernel
    single = dev_u16(plane)
    for i in range(n):
        ck(gpu_lib, gpu_lib.saber_k_paint_nearest(ptr(ld[i]), src[0], src[1], thr, labels[i], ptr(single), dst[0], dst[1], None, None))
    assert torch.equal(single, pd)
    # nothing above the threshold: the plane stays, the flag stays clear; without a flag pointer the call paints all the same
    pd2, flag2 = dev_u16(plane), torch.zeros(1, dtype=torch.int32, device="cuda")
    ck(gpu_lib, gpu_lib.saber_k_paint_nearest_stack(ptr(ld), n, src[0], src[1], lab, 1e9, ptr(pd2), dst[0], dst[1], ptr(flag2), None))
    assert np.array_equal(host_u16(pd2), plane) and int(flag2.item()) == 0
    ck(gpu_lib, gpu_lib.saber_k_paint_nearest_stack(ptr(ld), n, src[0], src[1], lab, thr, ptr(pd2), dst[0], dst[1], None, None))
    assert np.array_equal(host_u16(pd2), ref)


# ------------------------------------------------------------------------------------------------ relabel_frames
@pytest.mark.parametrize("L", [1, 2, 40, LUT_LDS, LUT_LDS + 1])
@pytest.mark.parametrize("HW", [37 * 53, 1, 7, 8, 9])
def test_relabel_frames(gpu_lib, HW, L):
    Z = 5
    rng = np.random.default_rng(HW * 31 + L)
    vol = rng.integers(0, min(max(2 * L, 4), 65536), (Z, HW)).astype(np.uint16)       # about half the values are >= L: they pass through
    vol[:, -1] = 65535
    if HW > 1:
        vol[:, 0] = L - 1
    lut = rng.integers(0, 65536, (Z, L)).astype(np.uint16)          # a different table per frame
    lut[0] = np.arange(L)                                           # an all-identity frame
    lut[1] = 0                                                      # an all-zero frame
    lut[2, : L // 2] = np.arange(L // 2)                            # partly identity: some vectors change, some do not
    ref = np.where(vol < L, np.take_along_axis(lut, np.minimum(vol, L - 1).astype(np.int64), axis=1), vol).astype(np.uint16)
    assert (vol >= L).any()
    vd, ld = dev_u16(vol), dev_u16(lut)
    assert vd.data_ptr() % 16 == 0                                  # so frames 1 and 3 start off the 16-byte boundary when HW is odd
    ck(gpu_lib, gpu_lib.saber_k_relabel_frames(ptr(vd), Z, HW, ptr(ld), L, None))
    assert np.array_equal(host_u16(vd), ref)


def test_relabel_frames_wrapper_applies_the_presence_filter(gpu_lib):
    from saber_amd.utils import labelvol, volprep
    rng = np.random.default_rng(5)
    Z, n = 6, 4
    vol = rng.integers(0, n + 1, (Z, 9, 11)).astype(np.uint16)
    bounds = rng.uniform(0, 1, (Z, n))
    bounds[2, 1] = 0.5                                              # equal to the threshold: kept
    ref = vol.copy()
    for z in range(Z):
        for mi in range(n):
            if float(bounds[z, mi]) < 0.5:
                ref[z][ref[z] == mi + 1] = 0
    vd = dev_u16(vol)
    out = labelvol.relabel_frames_(vd, volprep.to_device_volume(labelvol.presence_keep_table(bounds, 0.5), vd.device))
    assert out is vd and np.array_equal(host_u16(vd), ref) and (ref != vol).any()


# ------------------------------------------------------------------------------------------------ merges
@pytest.mark.parametrize("binarize", [0, 1])
@pytest.mark.parametrize("n", COUNTS)
def test_merge_max_u16(gpu_lib, n, binarize):
    rng = np.random.default_rng(n + binarize)
    acc = rng.choice(np.array([0, 0, 1, 2, 5, 40000], dtype=np.uint16), n)      # the accumulator already holds values above 1
    src = rng.choice(np.array([0, 0, 1, 3, 7, 65535], dtype=np.uint16), n)
    acc[0], src[0] = 2, 1
    ref = np.maximum(acc, (src > 0).astype(np.uint16) if binarize else src)
    ad, sd = dev_u16(acc), dev_u16(src)
    ck(gpu_lib, gpu_lib.saber_k_merge_max_u16(ptr(ad), ptr(sd), n, binarize, None))
    assert np.array_equal(host_u16(ad), ref)
    # pointers off the 16-byte boundary (a slice of a larger buffer)
    pad_a, pad_s = dev_u16(np.concatenate([[9], acc])), dev_u16(np.concatenate([[9], src]))
    ck(gpu_lib, gpu_lib.saber_k_merge_max_u16(ptr(pad_a[1:]), ptr(pad_s[1:]), n, binarize, None))
    assert np.array_equal(host_u16(pad_a), np.concatenate([[9], ref]))


def _class_ref(final, best, src, cls, conf):
    """the reference's per-mask loop (saber/segmenters/propagation.py:150-158): table entry idx + 1 belongs to mask idx"""
    for idx in range(len(cls) - 1):
        region = src == (idx + 1)
        if np.any(region):
            c = conf[idx + 1]
            upd = region & (c > best)
            final[upd] = cls[idx + 1]
            best[upd] = c


@pytest.mark.parametrize("n", COUNTS)
def test_merge_class_conf(gpu_lib, n):
    rng = np.random.default_rng(n)
    L = 6
    levels = np.array([0.0, 0.25, 0.5, 0.75, 0.9], dtype=np.float32)
    final = rng.integers(0, 3, n).astype(np.uint16)
    best = rng.choice(levels, n).astype(np.float32)
    fd, bd = dev_u16(final), torch.from_numpy(best).cuda()
    for call in range(2):                                           # two successive seed slices
        src = rng.integers(0, L + 3, n).astype(np.uint16)           # 0: untouched; >= L: ignored
        cls = rng.integers(1, 4, L).astype(np.uint16)
        conf = rng.choice(levels[1:], L).astype(np.float32)
        cls[0], conf[0] = 3, 100.0                                  # entry 0 would win everywhere if it were ever applied
        if call == 0:
            src[0], best[0], final[0] = 1, conf[1], 999             # a tie conf == best: must not update
            fd, bd = dev_u16(final), torch.from_numpy(best).cuda()
        if n >= 8:
            src[1], src[2] = 0, L                                   # label 0 and a label >= L
        f0 = final.copy()
        _class_ref(final, best, src, cls, conf)
        sd, cd, pd = dev_u16(src), dev_u16(cls), torch.from_numpy(conf).cuda()      # named: a temporary's block would be recycled for the next upload
        ck(gpu_lib, gpu_lib.saber_k_merge_class_conf(ptr(fd), ptr(bd), ptr(sd), ptr(cd), ptr(pd), L, n, None))
        torch.cuda.synchronize()
        assert np.array_equal(host_u16(fd), final) and np.array_equal(bd.cpu().numpy(), best)
        if call == 0:
            assert final[0] == 999
    if n == COUNTS[-1]:
        assert (final != f0).any()


def test_bad_arguments_return_the_error_status(gpu_lib):
    lg = torch.zeros((2, 4, 4), dtype=torch.float32, device="cuda")
    pl = torch.zeros((4, 4), dtype=torch.int16, device="cuda")
    bf = torch.zeros(16, dtype=torch.float32, device="cuda")
    ok = (C.c_int * 2)(1, 2)
    for args in ((ptr(lg), 2, 4, 4, ok, 0.0, ptr(pl), 0, 4, None, None),             # a non-positive shape
                 (ptr(lg), 2, 4, -1, ok, 0.0, ptr(pl), 4, 4, None, None),
                 (ptr(lg), 2, 4, 4, (C.c_int * 2)(1, 65536), 0.0, ptr(pl), 4, 4, None, None),      # a label above 65535
                 (ptr(lg), 2, 4, 4, (C.c_int * 2)(-1, 2), 0.0, ptr(pl), 4, 4, None, None)):
        assert gpu_lib.saber_k_paint_nearest_stack(*args) == -1
        assert gpu_lib.saber_k_last_error().decode().startswith("paint_nearest_stack:")
    assert gpu_lib.saber_k_relabel_frames(ptr(pl), 1, 16, ptr(pl), 0, None) == -1            # L <= 0
    assert gpu_lib.saber_k_last_error().decode().startswith("relabel_frames:")
    assert gpu_lib.saber_k_relabel_frames(ptr(pl), 0, 16, ptr(pl), 4, None) == -1
    assert gpu_lib.saber_k_relabel_frames(ptr(pl), 1, 0, ptr(pl), 4, None) == -1
    assert gpu_lib.saber_k_merge_class_conf(ptr(pl), ptr(bf), ptr(pl), ptr(pl), ptr(bf), 0, 16, None) == -1
    assert gpu_lib.saber_k_last_error().decode().startswith("merge_class_conf:")
    assert gpu_lib.saber_k_merge_max_u16(ptr(pl), ptr(pl), -1, 0, None) == -1
    assert gpu_lib.saber_k_last_error().decode().startswith("merge_max_u16:")
    torch.cuda.synchronize()
    assert not pl.any()                                             # none of the refused calls launched anything


# ------------------------------------------------------------------------------------------------ end to end: the adapter
@pytest.fixture(scope="module")
def video_case():
    """the case of tests/test_gpu_video.py: tiny trunk, seeded weights with a positive object-score bias (the seeded head otherwise
    predicts 'absent' on every frame), default_rng(42) tomogram of 7 frames, two disk seeds"""
    from saber_amd.adapters.sam2.video import VideoPredictor
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import param_specs, seeded_weights
    cfg = get_config("tiny")
    W = seeded_weights(cfg, 0, video=True)
    W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] = W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] + np.float32(3.0)
    img_keys = set(param_specs(cfg).keys())
    eng = Engine("tiny", device=0, weights={k: v for k, v in W.items() if k in img_keys}, max_images=3, max_prompts=8)
    vp = VideoPredictor(eng, W, num_maskmem=2)
    tomo = np.random.default_rng(42).uniform(-1, 1, (7, 128, 128)).astype(np.float32)
    yy, xx = np.mgrid[:128, :128]
    seed = ((yy - 64) ** 2 + (xx - 64) ** 2 < (128 // 6) ** 2).astype(np.float32)
    seed2 = ((yy - 40) ** 2 + (xx - 90) ** 2 < 14 ** 2).astype(np.float32)
    yield vp, tomo, [seed, seed2]
    eng.close()


def _metrics(ad):
    return {z: {o: dict(m) for o, m in per.items()} for z, per in ad.frame_metrics.items()}


def test_segment_volume_device_route_equals_host_route(video_case):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    vp, tomo, seeds = video_case
    ad = SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0")
    ad._video_predictor = vp
    ad.set_volume(tomo)

    def run(thr, **route):
        vol = ad.segment_volume(2, masks=seeds, min_presence_score=thr, **route)
        metrics, scores = _metrics(ad), ad.frame_scores.copy()
        ad.reset_state()
        return vol, metrics, scores

    host0, m0, s0 = run(0.0)
    again, m0b, s0b = run(0.0)
    # the exact comparison below rests on the tracking being repeatable run to run
    assert np.array_equal(host0, again) and m0 == m0b and np.array_equal(s0, s0b), "two host-route runs of the same case differ"
    assert host0.dtype == np.uint16 and host0.any()
    dev0, md0, sd0 = run(0.0, device_volume=True)
    assert isinstance(dev0, torch.Tensor) and dev0.is_cuda and dev0.dtype in (torch.int16, torch.uint16) and tuple(dev0.shape) == tomo.shape
    assert np.array_equal(host_u16(dev0), host0) and md0 == m0 and np.array_equal(sd0, s0)
    # a threshold strictly between two presence scores of (frame, object) pairs the unfiltered volume actually paints
    painted = sorted({m0[z][o]["presence_score"] for z in range(tomo.shape[0]) for o in m0[z] if (host0[z] == o).any()})
    print("presence scores of painted (frame, object) pairs:", painted)
    assert len(painted) >= 2, "the painted pairs share one presence score: no threshold separates them"
    gaps = [(b - a, a, b) for a, b in zip(painted[:-1], painted[1:])]
    _, lo, hi = max(gaps)
    thr = (lo + hi) / 2
    assert lo < thr < hi
    host1, m1, _ = run(thr)
    assert host1.any() and not np.array_equal(host1, host0), "the filter at this threshold changes nothing: the comparison would prove nothing"
    dev1, md1, _ = run(thr, device_volume=True)
    assert dev1.is_cuda and np.array_equal(host_u16(dev1), host1) and md1 == m1 == m0


# ------------------------------------------------------------------------------------------------ end to end: the segmenters
def _volume(Z=7, S=384):
    """the toy volume of tests/test_gpu_dropin.py"""
    rng = np.random.default_rng(11)
    vol = rng.normal(32768, 3000, (Z, S, S))
    zz, yy, xx = np.mgrid[:Z, :S, :S]
    for _ in range(9):
        cy, cx, r = rng.integers(40, S - 40, 2).tolist() + [int(rng.integers(15, 60))]
        vol[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += rng.choice([-6000, 6000])
    return np.clip(vol, 0, 65535).astype(np.float32)


def _amg():
    from saber_amd.adapters.sam2.amg import cfgAMG
    os.environ["SABER_AMD_SEEDED_WEIGHTS"] = "1"               # no checkpoint offline: deterministic synthetic weights
    return cfgAMG(npoints=8, crop_n_layers=0, pred_iou_thresh=0.2, stability_score_thresh=0.3, sam2_cfg="small")


def _both_routes(seg, call):
    out = []
    for route in (False, True):
        seg.device_volumes = route
        out.append(call())
    seg.device_volumes = False
    host, dev = out
    assert isinstance(host, np.ndarray) and isinstance(dev, np.ndarray)
    assert host.any(), "the host route found nothing: the case no longer exercises the path"
    assert dev.dtype == host.dtype and dev.shape == host.shape and np.array_equal(dev, host)
    return host


def test_propagation_single_segment_device_volumes():
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.segmenters.propagation import propagationSegmenter
    seg = propagationSegmenter(deviceID=0, cfg=SAM2AdapterConfig(cfg="tiny", amg_cfg=_amg(), min_mask_area=50), min_mask_area=50)
    seg.filter_threshold = -1.0                       # keep every frame: the untrained object-score head says nothing about presence
    vol = _volume()
    host = _both_routes(seg, lambda: seg.segment(vol, ini_depth=4))
    assert host.dtype == np.uint32 and host.shape == vol.shape
    # segment_3d hands the device tensor through
    seg.device_volumes = True
    masks = seg.segment_image(vol[2], display=False)
    m3 = seg.segment_3d(vol, [m["segmentation"] for m in masks], ann_frame_idx=2)
    assert isinstance(m3, torch.Tensor) and m3.is_cuda and tuple(m3.shape) == vol.shape


def test_multi_depth_tomo_segmenter_device_volumes():
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.segmenters.tomo import multiDepthTomoSegmenter
    seg = multiDepthTomoSegmenter(deviceID=0, cfg=SAM2AdapterConfig(cfg="tiny", amg_cfg=_amg(), min_mask_area=50), min_mask_area=50)
    seg.filter_threshold = -1.0
    vol = _volume()
    host = _both_routes(seg, lambda: seg.segment(vol, thickness=2, num_slabs=3, delta_z=2))
    assert host.dtype == np.uint32 and host.shape == vol.shape
    seg.device_volumes = True                         # tomoSegmenter.segment_vol hands the device tensor through
    out = seg.segment_vol(vol, 2, zSlice=3)
    assert isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == vol.shape


def test_propagation_multiclass_segment_device_volumes():
    from oracle import classifier_ref as cr
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.automask import get_engine
    from saber_amd.classifier.models.predictor import Predictor
    from saber_amd.segmenters.propagation import propagationSegmenter
    _amg()
    eng = get_engine("small", "cuda:0")
    pred = Predictor(None, None, config={"model": {"num_classes": 3}, "amg_params": {"sam2_cfg": "small", "npoints": 8, "crop_n_layers": 0,
                                                                                   "pred_iou_thresh": 0.2, "stability_score_thresh": 0.3}},
                     head_weights=cr.seeded_head(3, 0), engine=eng, min_area=50)
    ps = propagationSegmenter(deviceID=0, cfg=SAM2AdapterConfig(cfg="tiny", classifier=pred, min_mask_area=50), min_mask_area=50)
    ps.ini_depth, ps.target_class = 4, -1
    ps.filter_threshold = -1.0
    vol = _volume()
    host = _both_routes(ps, lambda: ps.multiclass_segment(vol))
    assert host.dtype == np.uint16 and host.shape == vol.shape and set(np.unique(host)) <= {0, 1, 2}
