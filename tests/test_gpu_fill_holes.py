"""GPU: hole filling of tracked masks (csrc/holefill.hip, VideoPredictor(fill_hole_area=...), SAM2AdapterConfig.fill_hole_area).
(a) saber_k_fill_holes on planes whose answer is known by construction, (b) on random planes against the host restatement
(tests/fill_holes_ref.py), (c) the tracking loop with the step on and off, (d) prompted frames, (e) the adapter.  Every comparison is
bit equality: the step copies or replaces pixels, and the kernels of the tracking loop are deterministic."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.fill_holes_cases import constructed_cases
from tests.fill_holes_ref import FILL_VALUE, fill_holes_ref, random_planes

pytestmark = pytest.mark.gpu

CASES = constructed_cases()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def fill_dev(lib, x, max_area, in_place=False, ws_bytes=None, expect=0):
    """saber_k_fill_holes on x (planes, H, W); returns the output plane(s) as numpy (out-of-place: the output starts as 7.0 everywhere)"""
    P, H, W = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = xd if in_place else torch.full_like(xd, 7.0)
    ws = torch.zeros(x.size * 8 if ws_bytes is None else max(ws_bytes, 4), dtype=torch.uint8, device="cuda")
    st = lib.saber_k_fill_holes(ptr(xd), P, H, W, max_area, 0.1, ptr(out), ptr(ws), x.size * 8 if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    assert st == expect, lib.saber_k_last_error().decode()
    if not in_place:
        assert same(xd, x)                                     # the input is read only
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ (a) constructed planes
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_constructed_planes(gpu_lib, case):
    name, x, max_area, expected = case
    got = fill_dev(gpu_lib, x, max_area)
    assert same(got, expected), f"{name}: {int((bits(got) != bits(expected)).sum())} pixels differ"
    assert same(fill_dev(gpu_lib, x, max_area, in_place=True), got)          # in place = out of place


def test_errors_write_nothing(gpu_lib):
    x = CASES[0][1]
    n = x.size
    for kw, word in ((dict(max_area=8, ws_bytes=n * 8 - 1), "workspace"), (dict(max_area=0), "max_area"), (dict(max_area=-3), "max_area")):
        got = fill_dev(gpu_lib, x, expect=-1, **kw)
        assert word in gpu_lib.saber_k_last_error().decode() and (got == 7.0).all()
    xd = torch.from_numpy(x).cuda()
    out, ws = torch.full_like(xd, 7.0), torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    P, H, W = x.shape
    for args in ((None, P, H, W, 8, 0.1, ptr(out), ptr(ws), n * 8), (ptr(xd), P, H, W, 8, 0.1, None, ptr(ws), n * 8),
                 (ptr(xd), P, H, W, 8, 0.1, ptr(out), None, n * 8), (ptr(xd), 0, H, W, 8, 0.1, ptr(out), ptr(ws), n * 8),
                 (ptr(xd), P, 0, W, 8, 0.1, ptr(out), ptr(ws), n * 8), (ptr(xd), P, H, -1, 8, 0.1, ptr(out), ptr(ws), n * 8),
                 (ptr(xd), 1 << 15, 1 << 8, 1 << 8, 8, 0.1, ptr(out), ptr(ws), 1 << 62)):          # 2^31 pixels
        assert gpu_lib.saber_k_fill_holes(*args, None) == -1
        assert gpu_lib.saber_k_last_error().decode().startswith("fill_holes:")
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    got = fill_dev(gpu_lib, x, 8, ws_bytes=n * 8)              # the documented size is enough
    assert same(got, CASES[0][3])


# ------------------------------------------------------------------------------------------------ (b) random planes
RANDOM = ((0, (3, 64, 64)), (1, (2, 37, 70)), (2, (1, 256, 256)), (3, (4, 33, 130)), (4, (16, 256, 256)))


@pytest.mark.parametrize("seed,shape", RANDOM, ids=[f"seed {s} {sh}" for s, sh in RANDOM])
def test_random_planes_against_restatement(gpu_lib, seed, shape):
    x = random_planes(seed, shape)
    ref, filled, kept = fill_holes_ref(x, 8)
    print(f"{shape}: the restatement fills {filled} components and keeps {kept}")
    assert filled >= 50 and kept >= 20
    got = fill_dev(gpu_lib, x, 8)
    assert same(got, ref), f"{int((bits(got) != bits(ref)).sum())} pixels differ"
    if seed == 0:
        for max_area in (1, 64):
            ref_a, f_a, k_a = fill_holes_ref(x, max_area)
            assert f_a >= 50 and k_a >= 1 and not same(ref_a, ref)
            assert same(fill_dev(gpu_lib, x, max_area), ref_a) and same(fill_dev(gpu_lib, x, max_area, in_place=True), ref_a)


# ------------------------------------------------------------------------------------------------ (c) - (e): the video path
def _disc():
    yy, xx = np.mgrid[:128, :128]
    return ((yy - 64) ** 2 + (xx - 64) ** 2 < (128 // 6) ** 2).astype(np.float32)


def _video_case(precision):
    """the recipe of tests/test_gpu_video.py::video_case (tiny trunk, seeded weights with a positive object-score bias, 7 frames of
    default_rng(42) noise, centred disc seed); two predictors on one handle: the step off (built without the argument) and on (8)"""
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import param_specs, seeded_weights
    from saber_amd.adapters.sam2.video import VideoPredictor, load_tomogram_frames
    cfg = get_config("tiny")
    W = seeded_weights(cfg, 0, video=True)
    W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] = W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] + np.float32(3.0)
    img_keys = set(param_specs(cfg).keys())
    kw = {} if precision == "bf16" else {"precision": precision}
    eng = Engine("tiny", device=0, weights={k: v for k, v in W.items() if k in img_keys}, max_images=3, max_prompts=8, **kw)
    plain = VideoPredictor(eng, W, num_maskmem=2)
    fill = VideoPredictor(eng, W, num_maskmem=2, fill_hole_area=8)
    assert plain.fill_hole_area == 0 and fill.fill_hole_area == 8 and fill.f16 == (precision == "fp16")
    tomo = np.random.default_rng(42).uniform(-1, 1, (7, 128, 128)).astype(np.float32)
    return {"eng": eng, "W": W, "plain": plain, "fill": fill, "tomo": tomo, "frames": load_tomogram_frames(tomo), "seed": _disc()}


@pytest.fixture(scope="module")
def case_bf16():
    c = _video_case("bf16")
    yield c
    c["eng"].close()


@pytest.fixture(scope="module")
def case_fp16():
    c = _video_case("fp16")
    yield c
    c["eng"].close()


def _host(o):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}


def _run_tracking(vp, frames, seeds, start=3, batch_objects=False):
    """add_new_mask on `start` for every seed, propagation both ways.  The two predictors of a case share the engine's slots, so a run
    starts with init_state and is finished before the other predictor's begins."""
    vp.batch_objects = batch_objects
    vp.init_state(frames)
    for i, s in enumerate(seeds, start=1):
        vp.add_new_mask(start, i, s)
    yielded = {}
    for rev in (False, True):
        for t, ids, logits in vp.propagate_in_video(start, None, reverse=rev):
            assert ids == list(range(1, len(seeds) + 1))
            yielded[(t, rev)] = logits.cpu()
    with torch.inference_mode():
        resized = {(oid, t): vp._resize(o["pred_masks"], 256, 256, *vp.video_hw).cpu()
                   for oid in vp.obj_ids for kind in ("cond", "non_cond") for t, o in vp.out[oid][kind].items()}
    torch.cuda.synchronize()
    state = {oid: {kind: {t: _host(o) for t, o in vp.out[oid][kind].items()} for kind in ("cond", "non_cond")} for oid in vp.obj_ids}
    return state, yielded, resized


def _tracking(case, seeds, batch_objects):
    Z, start = case["tomo"].shape[0], 3
    p_state, p_yield, _ = _run_tracking(case["plain"], case["frames"], seeds, start, batch_objects)
    assert case["plain"]._fill_ws is None                                    # off: nothing allocated
    f_state, f_yield, f_resized = _run_tracking(case["fill"], case["frames"], seeds, start, batch_objects)
    assert set(p_yield) == set(f_yield) and len(f_yield) == Z + 1
    changed = 0
    for oid in range(1, len(seeds) + 1):
        assert sorted(f_state[oid]["non_cond"]) == sorted(p_state[oid]["non_cond"]) == [t for t in range(Z) if t != start]
        for t in range(Z):
            rev = t < start
            if t == start:                                                   # the conditioning frame: a disc has no holes
                p, f = p_state[oid]["cond"][t], f_state[oid]["cond"][t]
                assert fill_holes_ref(p["pred_masks"].numpy(), 8)[1] == 0
                for k in ("pred_masks", "obj_ptr", "mem"):
                    assert same(p[k], f[k]), (oid, t, k)
                assert p["obj"] == f["obj"]
                for r in (False, True):
                    assert same(p_yield[(t, r)][oid - 1, 0], f_yield[(t, r)][oid - 1, 0])
                continue
            p, f = p_state[oid]["non_cond"][t], f_state[oid]["non_cond"][t]
            ref, n_filled, n_kept = fill_holes_ref(p["pred_masks"].numpy(), 8)
            n_px = int((bits(ref) != bits(p["pred_masks"])).sum())
            print(f"object {oid} frame {t}: {n_filled} components ({n_px} pixels) filled, {n_kept} kept")
            changed += n_px
            assert same(f["pred_masks"], ref), (oid, t)
            for k in ("obj_ptr", "mem"):                                     # the step runs after the memory encoder
                assert same(p[k], f[k]), (oid, t, k)
            assert p["obj"] == f["obj"]
            assert same(f_yield[(t, rev)][oid - 1, 0], f_resized[(oid, t)]), (oid, t)
    assert changed >= 1000
    return changed


def test_tracking_fills_after_the_memory_encoder(case_bf16):
    _tracking(case_bf16, [case_bf16["seed"]], False)


def test_tracking_fills_after_the_memory_encoder_fp16(case_fp16):
    _tracking(case_fp16, [case_fp16["seed"]], False)


def test_tracking_two_objects_batched(case_bf16):
    yy, xx = np.mgrid[:128, :128]
    seed2 = ((yy - 40) ** 2 + (xx - 90) ** 2 < 14 ** 2).astype(np.float32)
    try:
        _tracking(case_bf16, [case_bf16["seed"], seed2], True)
    finally:
        case_bf16["plain"].batch_objects = case_bf16["fill"].batch_objects = False


# ------------------------------------------------------------------------------------------------ (d) conditioning frames
def test_mask_prompt_with_holes(case_bf16):
    """a seed mask with a one-pixel and a 3 x 3 hole (at 128 px: about 2 x 2 and 6 x 6 low-resolution pixels): the small one is filled in
    what add_new_mask stores and returns, the large one stays, and the preflight encodes the memory from the filled logits"""
    c = case_bf16
    seed = c["seed"].copy()
    seed[60, 58] = 0
    seed[66:69, 68:71] = 0
    got = {}
    for name in ("plain", "fill"):
        vp = c[name]
        vp.init_state(c["frames"])
        _, ids, low = vp.add_new_mask(3, 1, seed)
        entry = vp.temp[1][3]
        assert low is entry["pred_masks"] and ids == [1]
        raw = entry["raw"]
        with torch.inference_mode():
            vp._preflight()
            o = vp.out[1]["cond"][3]
            mfm = vp._resize(o["pred_masks"], 256, 256, 1024, 1024, antialias=0, post=2, a=20.0, c=-10.0)
            again = vp._encode_memory(raw, mfm, True)
        torch.cuda.synchronize()
        got[name] = (low.cpu(), o["pred_masks"].cpu(), o["mem"].cpu(), again.cpu(), o["obj_ptr"].cpu())
        vp.reset_state()
    p_low, f_low = got["plain"][0], got["fill"][0]
    ref, n_filled, n_kept = fill_holes_ref(p_low.numpy(), 8)
    n_px = int((bits(ref) != bits(p_low)).sum())
    print(f"seed with holes: {n_filled} components ({n_px} pixels) filled, {n_kept} kept")
    assert n_px >= 1 and same(f_low, ref) and same(got["fill"][1], ref) and same(got["plain"][1], p_low)
    assert (ref[120:122, 116:118] == FILL_VALUE).all() and (p_low.numpy()[120:122, 116:118] <= 0).all()      # the one-pixel hole
    assert (f_low.numpy()[132:138, 136:142] <= 0).any()                                                        # the large hole stays
    assert not same(got["fill"][2], got["plain"][2])                          # the memory saw the filled mask
    assert same(got["fill"][2], got["fill"][3]) and same(got["plain"][2], got["plain"][3])
    assert same(got["fill"][4], got["plain"][4])                              # the pointer comes from the mask itself


def test_clicks_see_the_filled_logits(case_fp16):
    """add_new_points_or_box on an untracked frame: the stored / returned output of one click is the restatement of the plain run's, and
    a second click (clear_old_points=False) decodes with the FILLED logits as its mask prompt"""
    c = case_fp16
    eng = c["eng"]
    click1, click2 = dict(points=[[512.0, 500.0]], labels=[1]), dict(points=[[650.0, 300.0]], labels=[0], clear_old_points=False)
    eng.set_multipoint(True)                                                  # two clicks are 16 decoder tokens
    try:
        def run(vp, swap_in=None):
            vp.init_state(c["frames"], video_hw=(1024, 1024))
            _, _, v1 = vp.add_new_points_or_box(3, 1, **click1)
            low1 = vp.temp[1][3]["pred_masks"]
            with torch.inference_mode():
                r1 = vp._resize(low1, 256, 256, 1024, 1024)
            if swap_in is not None:
                vp.temp[1][3]["pred_masks"] = torch.from_numpy(swap_in).to(vp.dev)
            _, _, v2 = vp.add_new_points_or_box(3, 1, **click2)
            low2 = vp.temp[1][3]["pred_masks"]
            torch.cuda.synchronize()
            res = (low1.cpu(), v1[0, 0].cpu(), r1.cpu(), low2.cpu(), v2[0, 0].cpu())
            vp.reset_state()
            return res

        p1, pv1, pr1, p2, _ = run(c["plain"])
        f1, fv1, fr1, f2, fv2 = run(c["fill"])
        ref1, n1, _ = fill_holes_ref(p1.numpy(), 8)
        assert n1 >= 1 and same(f1, ref1) and same(fv1, fr1) and same(pv1, pr1) and not same(fv1, pv1)
        s1, sv1, _, s2, _ = run(c["plain"], swap_in=ref1)                     # the plain predictor, prompted with the filled plane
        assert same(s1, p1)
        ref2, n2, _ = fill_holes_ref(s2.numpy(), 8)
        print(f"first click: {n1} components filled; second click: {n2}")
        assert same(f2, ref2)
        assert not same(s2, p2)                                               # ... which is not what the unfilled prompt gives
    finally:
        eng.set_multipoint(False)


# ------------------------------------------------------------------------------------------------ (e) adapter
def _nearest(video_logits):
    """the label plane saber_k_paint_nearest paints from 1024-px logits on a 128-px slice: source pixel floor((i + 0.5) * 8)"""
    return (video_logits[4::8, 4::8] > 0).numpy()


def test_adapter_segment_volume(case_bf16, monkeypatch):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    c = case_bf16
    monkeypatch.delenv("SABER_AMD_FILL_HOLE_AREA", raising=False)
    vols, lows = {}, {}
    for name, config in (("plain", SAM2AdapterConfig(cfg="tiny")), ("fill", SAM2AdapterConfig(cfg="tiny", fill_hole_area=8))):
        ad = SAM2Adapter(config, device="cuda:0")
        assert ad._fill_hole_area() == c[name].fill_hole_area
        ad._video_predictor = c[name]                                         # the case's weights (object-score bias)
        ad.set_volume(c["tomo"])
        vols[name] = ad.segment_volume(3, masks=[c["seed"]], min_presence_score=0.0)
        vp = c[name]
        with torch.inference_mode():
            lows[name] = {t: (o["pred_masks"].cpu(), vp._resize(o["pred_masks"], 256, 256, 1024, 1024).cpu())
                          for kind in ("cond", "non_cond") for t, o in vp.out[1][kind].items()}
        vp.reset_state()
    differ = 0
    for t in range(c["tomo"].shape[0]):
        assert same(lows["fill"][t][0], fill_holes_ref(lows["plain"][t][0].numpy(), 8)[0])
        for name in ("plain", "fill"):                                        # a frame of the volume is its stored logits, resized and thresholded
            assert np.array_equal(vols[name][t] > 0, _nearest(lows[name][t][1])), (name, t)
        differ += int((vols["fill"][t] != vols["plain"][t]).sum())
    assert np.array_equal(vols["fill"][3], vols["plain"][3])                  # the seeded frame
    print(f"voxels that differ between the volumes: {differ}")
    assert differ > 0


def test_adapter_config_reaches_the_predictor(monkeypatch):
    """SAM2Adapter._video() as `saber segment tomograms` builds it: the config's value arrives, and the default route (no value, no
    environment) gives the predictor one gets without the argument - same volume, nothing allocated for the step"""
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    from saber_amd.adapters.sam2.video import VideoPredictor
    from saber_amd import pretrained_weights
    monkeypatch.delenv("SABER_AMD_FILL_HOLE_AREA", raising=False)
    monkeypatch.setenv("SABER_AMD_SEEDED_WEIGHTS", "1")
    assert SAM2Adapter(SAM2AdapterConfig(cfg="tiny", fill_hole_area=8), device="cuda:0")._video().fill_hole_area == 8
    monkeypatch.setenv("SABER_AMD_FILL_HOLE_AREA", "8")
    assert SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0")._video().fill_hole_area == 8
    monkeypatch.delenv("SABER_AMD_FILL_HOLE_AREA")
    ad = SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0")
    vp = ad._video()
    assert vp.fill_hole_area == 0
    tomo = np.random.default_rng(42).uniform(-1, 1, (4, 128, 128)).astype(np.float32)
    ad.set_volume(tomo)
    vol = ad.segment_volume(1, masks=[_disc()], min_presence_score=0.0)
    assert vp._fill_ws is None
    ad2 = SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0")
    ad2._video_predictor = VideoPredictor(vp.eng, pretrained_weights.load_weights("tiny", None, video=True), num_maskmem=2)
    ad2.set_volume(tomo)
    assert np.array_equal(ad2.segment_volume(1, masks=[_disc()], min_presence_score=0.0), vol)
