"""GPU: non-overlapping masks of the video path (saber_k_resize_planes_non_overlap, VideoPredictor(non_overlap_masks=True),
SAM2Adapter.segment_volume(non_overlap_masks=True)).  (a) the kernel against saber_k_resize_plane per plane followed by the host
restatement (tests/non_overlap_ref.py), (b) the tracking loop on its three routes with the option on against the restatement of what it
yields with the option off, (c) _frame_output with an absent object, (d) the adapter's two volume routes, (e) the environment default.
Every comparison is bit equality: the constraint copies a value or replaces it by min(value, -10), and the resized value is specified as
the per-plane kernel's bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.non_overlap_ref import SUPPRESS_MAX, non_overlap_ref, overlap_pixels

pytestmark = pytest.mark.gpu

CANARY = 0x7FC12345                # a NaN no resize of finite planes produces


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def ck(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()


# ------------------------------------------------------------------------------------------------ (a) the kernel
def plain_resize(lib, xd, Ho, Wo):
    """saber_k_resize_plane (bilinear, no post transform), one call per plane"""
    n, H, W = xd.shape
    out = torch.empty((n, Ho, Wo), dtype=torch.float32, device="cuda")
    for i in range(n):
        ck(lib, lib.saber_k_resize_plane(ptr(xd[i]), 1, H, W, ptr(out[i]), Ho, Wo, 0, 0, 0.0, 0.0, None))
    return out


def constrained_resize(lib, xd, Ho, Wo, n=None):
    """the new entry on the first n planes of xd into a canary-filled output; returns the whole output as int32 bit patterns"""
    n_all, H, W = xd.shape
    out = torch.full((n_all, Ho, Wo), CANARY, dtype=torch.int32, device="cuda")
    ck(lib, lib.saber_k_resize_planes_non_overlap(ptr(xd), n_all if n is None else n, H, W, ptr(out), Ho, Wo, float(SUPPRESS_MAX), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def data_sets(n, H, W, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, H, W)) * 8).astype(np.float32)
    sets = {"random": x}
    if n >= 2:
        tie = (rng.standard_normal((n, H, W)) * 8).astype(np.float32)
        tie[0] += 16                                       # high enough to be the maximum at many pixels, also among 40 planes
        tie[min(2, n - 1)] = tie[0]                        # planes 0 and 2 identical (0 and 1 when there are two): the tie goes to plane 0
        sets["tie"] = tie
    sets["low"] = (-11.0 - np.abs(rng.standard_normal((n, H, W))) * 8).astype(np.float32)      # nothing above -10: nothing to suppress
    return sets


SHAPES = (((8, 8), (13, 11)),              # non-integer ratio, odd width: the scalar kernel
          ((8, 8), (8, 8)),                # identity
          ((16, 12), (5, 7)),              # down-sampling without the antialias filter
          ((256, 256), (300, 200)),
          ((256, 256), (512, 512)))        # the 16-byte store path, several blocks


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{a[0]}x{a[1]}->{b[0]}x{b[1]}" for a, b in SHAPES])
def test_kernel_is_the_plane_resize_then_the_restatement(gpu_lib, shape):
    (H, W), (Ho, Wo) = shape
    for n in (1, 2, 3, 17, 40):            # beyond object_batch (16) and any chunk of it
        for name, x in data_sets(n, H, W, 1000 * n + H + Wo).items():
            xd = torch.from_numpy(x).cuda()
            plain = plain_resize(gpu_lib, xd, Ho, Wo).cpu().numpy()
            ref = non_overlap_ref(plain)
            got = constrained_resize(gpu_lib, xd, Ho, Wo)
            bad = int((got != bits(ref)).sum())
            assert bad == 0, f"{name}, {n} planes: {bad} of {got.size} values differ ({int((got == CANARY).sum())} not written)"
            assert same(xd, x)                                                   # the input is read only
            if n == 1 or name == "low":
                assert same(ref, plain)                                          # one plane / nothing above -10: the plain resize
            elif name == "random":
                assert overlap_pixels(plain) > 0 and overlap_pixels(ref) == 0    # there was something to do
            else:
                k = min(2, n - 1)
                twin = (plain[0] >= plain.max(axis=0)) & (plain[0] > SUPPRESS_MAX)
                assert twin.any() and same(plain[0], plain[k])                   # pixels where the twins are the maximum:
                assert np.array_equal(ref[0][twin], plain[0][twin]) and (ref[k][twin] == SUPPRESS_MAX).all()      # plane 0 keeps it


def test_no_planes_is_no_launch(gpu_lib):
    xd = torch.randn((3, 8, 8), device="cuda")
    got = constrained_resize(gpu_lib, xd, 13, 12, n=0)
    assert (got == CANARY).all()
    got = constrained_resize(gpu_lib, xd, 13, 12, n=2)         # fewer planes than the buffers hold: the third stays untouched
    assert (got[2] == CANARY).all() and not (got[:2] == CANARY).any()


def test_refusals_write_nothing(gpu_lib):
    lib = gpu_lib
    xd = torch.randn((2, 8, 8), device="cuda")
    out = torch.full((2, 8, 8), CANARY, dtype=torch.int32, device="cuda")
    for args in ((None, 2, 8, 8, ptr(out), 8, 8), (ptr(xd), 2, 8, 8, None, 8, 8), (ptr(xd), -1, 8, 8, ptr(out), 8, 8), (ptr(xd), 2, 0, 8, ptr(out), 8, 8),
                 (ptr(xd), 2, 8, 8, ptr(out), 8, 0), (ptr(xd), 2, 8, 8, ptr(out), -1, 8)):
        assert lib.saber_k_resize_planes_non_overlap(*args, -10.0, None) == -1
        assert lib.saber_k_last_error().decode().startswith("resize_planes_non_overlap:")
    torch.cuda.synchronize()
    assert (out == CANARY).all()


# ------------------------------------------------------------------------------------------------ (b) - (e): the video path
def _disc(cy, cx, r):
    yy, xx = np.mgrid[:128, :128]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 < r ** 2).astype(np.float32)


# two overlapping discs and a third nested in the first; (centre y, centre x, radius) on the 128-px slice
DISCS = ((64, 52, 21), (64, 78, 20), (58, 44, 8))
START = 2
ROUTES = {"per object": (False, False), "batched attention": (True, False), "batched tail": (True, True)}


@pytest.fixture(scope="module")
def case():
    """the recipe of tests/test_gpu_video_batch.py::batch_case (tiny trunk, seeded video weights with the +3 object-score bias,
    num_maskmem = 2, windows of 3 frames) on a (5, 128, 128) tomogram; one engine with two predictors on it: the option off / on"""
    from saber_amd.adapters.sam2.video import VideoPredictor, load_tomogram_frames
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import param_specs, seeded_weights
    cfg = get_config("tiny")
    W = seeded_weights(cfg, 0, video=True)
    W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] = W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] + np.float32(3.0)
    img = {k: v for k, v in W.items() if k in set(param_specs(cfg).keys())}
    eng = Engine("tiny", device=0, weights=img, max_images=3, max_prompts=8)
    off = VideoPredictor(eng, W, num_maskmem=2, non_overlap_masks=False)
    on = VideoPredictor(eng, W, num_maskmem=2, non_overlap_masks=True)
    assert on.non_overlap_masks is True and off.non_overlap_masks is False
    tomo = np.random.default_rng(42).uniform(-1, 1, (5, 128, 128)).astype(np.float32)
    yield {"eng": eng, "W": W, "off": off, "on": on, "tomo": tomo, "frames": load_tomogram_frames(tomo), "seeds": [_disc(*d) for d in DISCS]}
    eng.close()


def _u16(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _run(vp, frames, seeds, route):
    """the seeds on frame START, propagation forwards then backwards; what the run yields and stores, on the host"""
    was = vp.batch_objects, vp.batch_tail
    vp.batch_objects, vp.batch_tail = ROUTES[route]
    try:
        vp.init_state(frames, video_hw=(128, 128))
        for i, m in enumerate(seeds, start=1):
            vp.add_new_mask(START, i, m)
        yielded = {}
        for reverse in (False, True):
            for t, ids, logits in vp.propagate_in_video(START, None, reverse):
                assert ids == list(range(1, len(seeds) + 1)) and tuple(logits.shape) == (len(seeds), 1, 128, 128)
                yielded[(t, reverse)] = logits.cpu().numpy()
        stored = {(oid, kind, t): (o["pred_masks"].cpu(), o["obj_ptr"].cpu(), float(o["obj"]), _u16(o["mem"]).cpu())
                  for oid in vp.obj_ids for kind in ("cond", "non_cond") for t, o in vp.out[oid][kind].items()}
        torch.cuda.synchronize()
    finally:
        vp.batch_objects, vp.batch_tail = was
    return yielded, stored


@pytest.mark.parametrize("route", list(ROUTES))
def test_yields_are_the_restatement_of_the_unconstrained_yields(case, route):
    y_off, s_off = _run(case["off"], case["frames"], case["seeds"], route)
    y_on, s_on = _run(case["on"], case["frames"], case["seeds"], route)
    Z = case["tomo"].shape[0]
    assert set(y_on) == set(y_off) == {(t, False) for t in range(START, Z)} | {(t, True) for t in range(START + 1)}
    tracked_overlap = 0
    for key in sorted(y_off):
        ref = non_overlap_ref(y_off[key])
        assert same(y_on[key], ref), (route, key, int((bits(y_on[key]) != bits(ref)).sum()))
        assert overlap_pixels(y_on[key]) == 0 and ((y_on[key] > SUPPRESS_MAX).sum(axis=0) <= 1).all()
        if key[0] == START:
            assert overlap_pixels(y_off[key]) >= 50                # the seeds overlap: the option has something to decide
            assert not same(y_on[key], y_off[key])
        else:
            tracked_overlap += overlap_pixels(y_off[key])
    print(f"{route}: pixels with two or more positive objects on the tracked frames, option off: {tracked_overlap}")
    # nothing that is stored changes: memories, pointers and the low-resolution logits are those of the unconstrained run
    assert set(s_on) == set(s_off) and any(k[1] == "non_cond" for k in s_on)
    for k in s_off:
        for a, b, what in zip(s_on[k], s_off[k], ("pred_masks", "obj_ptr", "obj", "mem")):
            assert (a == b) if what == "obj" else (a.dtype == b.dtype and torch.equal(a, b)), (route, k, what)


def test_frame_output_with_an_absent_object(case):
    """a fourth object with an input on another frame only: on frame START its plane is NO_OBJ_SCORE, the other three are the constrained
    three-object stack - which is also what the constraint over all four planes gives"""
    from saber_amd.adapters.sam2.video import NO_OBJ_SCORE
    got = {}
    for name in ("off", "on"):
        vp = case[name]
        vp.init_state(case["frames"], video_hw=(128, 128))
        for i, m in enumerate(case["seeds"], start=1):
            vp.add_new_mask(START, i, m)
        with torch.inference_mode():
            three = vp._frame_output(START)[2].cpu().numpy()
        vp.add_new_mask(4, 4, _disc(30, 100, 10))
        with torch.inference_mode():
            t, ids, four = vp._frame_output(START)
            other = vp._frame_output(4)[2].cpu().numpy()
        assert (t, ids) == (START, [1, 2, 3, 4]) and tuple(four.shape) == (4, 1, 128, 128)
        got[name] = (three, four.cpu().numpy(), other)
        vp.reset_state()
    three_off, four_off, other_off = got["off"]
    three_on, four_on, other_on = got["on"]
    assert overlap_pixels(three_off) >= 50 and same(four_off[:3], three_off) and (four_off[3] == NO_OBJ_SCORE).all()
    assert (four_on[3] == np.float32(NO_OBJ_SCORE)).all()
    assert same(three_on, non_overlap_ref(three_off)) and same(four_on[:3], three_on)
    assert same(four_on, non_overlap_ref(four_off))
    # frame 4: three absent objects and one present one - the plain resize of the present one
    assert (other_on[:3] == np.float32(NO_OBJ_SCORE)).all() and same(other_on, other_off) and (other_on[3] > 0).any()


def _nearest(video_logits):
    """the samples saber_k_paint_nearest reads from 1024-px logits for a 128-px slice: source pixel floor((i + 0.5) * 8)"""
    return video_logits[..., 4::8, 4::8]


def _paint(stack):
    """numpy paint of a frame: objects in order, label = object id where its logit is positive"""
    plane = np.zeros(stack.shape[-2:], np.uint16)
    for i in range(stack.shape[0]):
        plane[stack[i] > 0] = i + 1
    return plane


def test_adapter_segment_volume(case, monkeypatch):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    monkeypatch.delenv("SABER_AMD_NON_OVERLAP_MASKS", raising=False)
    vp = case["off"]
    ad = SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0")
    ad._video_predictor = vp                                              # the case's weights; the keyword switches the option per call
    Z = case["tomo"].shape[0]
    vols, scores, sampled = {}, {}, None
    for name, kw in (("off", {}), ("on", {"non_overlap_masks": True}), ("on device", {"non_overlap_masks": True, "device_volume": True}), ("after", {})):
        ad.set_volume(case["tomo"])
        vol = ad.segment_volume(START, masks=case["seeds"], min_presence_score=0.0, **kw)
        assert vp.non_overlap_masks is False                              # restored after the call
        vols[name] = vol.cpu().numpy().view(np.uint16).copy() if kw.get("device_volume") else vol.copy()
        scores[name] = ad.frame_scores.copy()
        if sampled is None:         # the unconstrained video-resolution logits of every frame, from what the tracker stored, at the paint's samples
            with torch.inference_mode():
                sampled = [_nearest(vp._resize_planes(torch.stack([(vp.out[o]["cond"].get(t) or vp.out[o]["non_cond"][t])["pred_masks"] for o in (1, 2, 3)], 0),
                                                      1024, 1024)).cpu().numpy() for t in range(Z)]
        vp.reset_state()
    assert vols["on"].shape == case["tomo"].shape and np.array_equal(vols["on"], vols["on device"])
    assert np.array_equal(vols["after"], vols["off"])                     # a call without the keyword runs with the option off again
    for name in ("on", "on device", "after"):
        assert np.array_equal(scores[name], scores["off"]), name
    assert scores["off"].shape == (Z, 3) and scores["off"].any()
    for t in range(Z):
        assert np.array_equal(vols["off"][t], _paint(sampled[t])), t
        assert np.array_equal(vols["on"][t], _paint(non_overlap_ref(sampled[t]))), t
    # the seeded frame: well inside an overlap the seeds tie at the same logit, so the lowest id wins where the paint order gave the highest
    (ay, ax, ar), (by, bx, br), (cy, cx, cr) = DISCS
    ab = (_disc(ay, ax, ar - 3) * _disc(by, bx, br - 3) * (1 - _disc(cy, cx, cr + 3))).astype(bool)
    ac = (_disc(ay, ax, ar - 3) * _disc(cy, cx, cr - 3)).astype(bool)
    assert ab.sum() >= 20 and ac.sum() >= 20
    on, off = vols["on"][START], vols["off"][START]
    assert (on[ab] == 1).all() and (off[ab] == 2).all() and (on[ac] == 1).all() and (off[ac] == 3).all()
    differ = [int((vols["on"][t] != vols["off"][t]).sum()) for t in range(Z)]
    print(f"voxels that differ between the volumes, per frame: {differ}")
    assert differ[START] >= int(ab.sum() + ac.sum())


def test_environment_default(case, monkeypatch):
    from saber_amd.adapters.sam2.video import VideoPredictor
    eng, W = case["eng"], case["W"]
    monkeypatch.setenv("SABER_AMD_NON_OVERLAP_MASKS", "1")
    assert VideoPredictor(eng, W, num_maskmem=2).non_overlap_masks is True
    assert VideoPredictor(eng, W, num_maskmem=2, non_overlap_masks=False).non_overlap_masks is False
    monkeypatch.setenv("SABER_AMD_NON_OVERLAP_MASKS", "0")
    assert VideoPredictor(eng, W, num_maskmem=2).non_overlap_masks is False
    monkeypatch.delenv("SABER_AMD_NON_OVERLAP_MASKS")
    assert VideoPredictor(eng, W, num_maskmem=2).non_overlap_masks is False
    assert VideoPredictor(eng, W, num_maskmem=2, non_overlap_masks=True).non_overlap_masks is True
