"""GPU: the frame-feature store of the video path (VideoPredictor(frame_store_gb=...), SAM2AdapterConfig.frame_store_gb): every frame of a
volume goes through the encoder once, whatever the number of seeds, directions and slabs, and every result is what the route without the
store gives, BIT FOR BIT - the stored features are copies (saber_export_slots / saber_import_slots) of what the same kernels computed from
the same frames.  Ten frames and encoder windows of four make windows that do not line up between seeds: a slot or row mix-up shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Z, S, WINDOW = 10, 128, 4
FULL = ((5, None), (2, None))            # (seed frame, max_frame_num_to_track) of the two propagations of a run; reset_state() between them


@pytest.fixture(scope="module")
def case():
    """tiny trunk, seeded weights with a positive object-score bias (as tests/test_gpu_video.py), encoder windows of 4 frames; the run
    without the store (seeds on frames 5 then 2, forward and backward) is computed once and shared"""
    from saber_amd.adapters.sam2.video import VideoPredictor, load_tomogram_frames
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import param_specs, seeded_weights
    cfg = get_config("tiny")
    W = seeded_weights(cfg, 0, video=True)
    k = "sam_mask_decoder.pred_obj_score_head.layers.2.bias"
    W[k] = W[k] + np.float32(3.0)
    img_keys = set(param_specs(cfg).keys())
    eng = Engine("tiny", device=0, weights={n: v for n, v in W.items() if n in img_keys}, max_images=WINDOW, max_prompts=8)
    tomo = np.random.default_rng(42).uniform(-1, 1, (Z, S, S)).astype(np.float32)
    yy, xx = np.mgrid[:S, :S]
    seed = ((yy - S // 2) ** 2 + (xx - S // 2) ** 2 < (S // 6) ** 2).astype(np.float32)
    frames = load_tomogram_frames(tomo)

    def predictor(gb):
        return VideoPredictor(eng, W, num_maskmem=2, frame_store_gb=gb)

    off = predictor(0)
    off.init_state(frames)
    ref = _run(off, seed, FULL)
    assert off.encoded_frames >= 2 * Z and off.restored_frames == 0 and off.stored_frames == 0 and off.store_bytes == 0
    yield {"predictor": predictor, "frames": frames, "seed": seed, "ref": ref, "tomo": tomo}
    eng.close()


def _run(vp, seed, plan, first=True):
    """the propagations of `plan` on the loaded volume: per propagation (every yielded logits tensor, every tracked frame's stored output)"""
    res = []
    for i, (start, n) in enumerate(plan):
        if i or not first:
            vp.reset_state()
        vp.add_new_mask(start, 1, seed)
        got = {}
        for rev in (False, True):
            for t, ids, logits in vp.propagate_in_video(start, n, reverse=rev):
                assert ids == [1]
                got[(t, rev)] = logits.clone()
        kept = {t: {"pred_masks": o["pred_masks"].clone(), "obj_ptr": o["obj_ptr"].clone(), "obj": o["obj"]} for t, o in vp.out[1]["non_cond"].items()}
        res.append((got, kept))
    torch.cuda.synchronize()
    return res


def _assert_same(got, ref):
    assert len(got) == len(ref)
    for (g_out, g_kept), (r_out, r_kept) in zip(got, ref):
        assert set(g_out) == set(r_out) and set(g_kept) == set(r_kept) and len(r_kept) > 0
        for key in r_out:
            assert torch.equal(g_out[key], r_out[key]), f"yielded logits of frame {key[0]} (reverse={key[1]})"
        for t in r_kept:
            assert torch.equal(g_kept[t]["pred_masks"], r_kept[t]["pred_masks"]), f"pred_masks of frame {t}"
            assert torch.equal(g_kept[t]["obj_ptr"], r_kept[t]["obj_ptr"]), f"obj_ptr of frame {t}"
            assert g_kept[t]["obj"] == r_kept[t]["obj"], f"object score of frame {t}"


def test_two_seeds_full_tracking(case):
    from saber_amd.adapters.sam2.video import FRAME_STORE_BYTES
    ref = case["ref"]
    assert len(ref[0][1]) == Z - 1 and len(ref[1][1]) == Z - 1          # every frame but the seed's was tracked, both times
    assert any(o["obj"] > 0 for o in ref[1][1].values())                 # real masks, not the NO_OBJ constant
    on = case["predictor"](1)
    assert on.store_bytes == 0                                            # allocated on first use
    on.init_state(case["frames"])
    _assert_same(_run(on, case["seed"], FULL), ref)
    assert on.encoded_frames == Z and on.restored_frames > 0
    assert on.stored_frames == Z and on.store_bytes == Z * FRAME_STORE_BYTES          # rows are capped at the volume's frames
    on.drop_frame_store()
    assert on.stored_frames == 0 and on.store_bytes == 0


def test_partial_coverage(case):
    plan = ((5, 2), (2, None))
    off = case["predictor"](0)
    off.init_state(case["frames"])
    ref = _run(off, case["seed"], plan)
    assert set(ref[0][1]) == {3, 4, 6, 7}
    on = case["predictor"](1)
    on.init_state(case["frames"])
    _assert_same(_run(on, case["seed"], plan), ref)
    assert on.encoded_frames == Z and on.stored_frames == Z


def test_budget_of_three_frames(case):
    from saber_amd.adapters.sam2.video import FRAME_STORE_BYTES
    on = case["predictor"](3 * 16 / 1024)
    assert on.frame_store_budget == 3 * FRAME_STORE_BYTES
    on.init_state(case["frames"])
    _assert_same(_run(on, case["seed"], FULL), case["ref"])
    assert on.stored_frames == 3
    assert 0 < on.store_bytes <= on.frame_store_budget
    assert Z < on.encoded_frames                                          # windows with a frame that got no row were encoded as before


def test_volume_identity(case):
    frames, seed, ref = case["frames"], case["seed"], case["ref"]
    on = case["predictor"](1)
    on.init_state(frames)
    before = on.encoded_frames
    first = _run(on, seed, FULL[:1])
    _assert_same(first, ref[:1])
    assert on.encoded_frames - before == Z
    # a fresh, bit-equal copy of the frames: the store is kept and the next propagation encodes nothing
    before = on.encoded_frames
    on.init_state(frames.copy())
    assert on.stored_frames == Z
    _assert_same(_run(on, seed, FULL[1:]), ref[1:])
    assert on.encoded_frames - before == 0
    # one voxel changed: the store goes, and the results are those of a fresh predictor on that volume
    changed = frames.copy()
    changed[3, 500, 700] += np.float32(0.5)
    before = on.encoded_frames
    on.init_state(changed)
    assert on.stored_frames == 0
    got = _run(on, seed, FULL[1:])
    assert on.encoded_frames - before == Z
    fresh = case["predictor"](0)
    fresh.init_state(changed)
    want = _run(fresh, seed, FULL[1:])
    _assert_same(got, want)
    # a device tensor the caller changes in place afterwards cannot reach the stack the store belongs to
    dev = torch.from_numpy(frames).cuda()
    on.init_state(dev)
    assert on.stored_frames == 0
    _assert_same(_run(on, seed, FULL[:1]), ref[:1])
    dev[3, 500, 700] += 0.5
    on.init_state(dev)
    assert on.stored_frames == 0
    _assert_same(_run(on, seed, FULL[1:]), want)


def test_adapter(case, monkeypatch):
    monkeypatch.setenv("SABER_AMD_SEEDED_WEIGHTS", "1")                   # no checkpoint offline: deterministic synthetic weights
    monkeypatch.delenv("SABER_AMD_VIDEO_STORE_GB", raising=False)
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    yy, xx = np.mgrid[:S, :S]
    seeds = [case["seed"], ((yy - 30) ** 2 + (xx - 90) ** 2 < 15 ** 2).astype(np.float32)]
    got = {}
    for name, config in (("off", SAM2AdapterConfig(cfg="tiny")), ("on", SAM2AdapterConfig(cfg="tiny", frame_store_gb=1))):
        ad = SAM2Adapter(config, device="cuda:0")
        vp = ad._video()
        assert vp.frame_store_budget == (2 ** 30 if name == "on" else 0)
        before = vp.encoded_frames
        ad.set_volume(case["tomo"])
        runs = []
        for start, batched in ((5, None), (2, True)):
            vol = ad.segment_volume(start, masks=seeds, min_presence_score=0.0, batch_objects=batched)
            runs.append((vol.copy(), ad.frame_scores.copy()))
            ad.reset_state()
        got[name] = runs
        if name == "on":
            assert vp.encoded_frames - before == Z and vp.restored_frames > 0 and vp.stored_frames == Z
        else:
            assert vp.encoded_frames - before > Z and vp.stored_frames == 0
        vp.drop_frame_store()
    for (v_off, s_off), (v_on, s_on) in zip(got["off"], got["on"]):
        assert v_off.shape == (Z, S, S) and v_off.any() and s_off.shape == (Z, 2) and np.abs(s_off).sum() > 0
        assert np.array_equal(v_off, v_on)
        assert np.array_equal(s_off, s_on)


def _volume(Z=7, S=384):
    """the toy volume of tests/test_gpu_dropin.py"""
    rng = np.random.default_rng(11)
    vol = rng.normal(32768, 3000, (Z, S, S))
    zz, yy, xx = np.mgrid[:Z, :S, :S]
    for _ in range(9):
        cy, cx, r = rng.integers(40, S - 40, 2).tolist() + [int(rng.integers(15, 60))]
        vol[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += rng.choice([-6000, 6000])
    return np.clip(vol, 0, 65535).astype(np.float32)


def test_multi_depth_segmenter(monkeypatch):
    """multiDepthTomoSegmenter prepares the volume once per call, so every slab's set_volume loads bit-equal frames and the store carries
    over: the frames go through the video model's encoder once for the three slabs, and the labels do not change"""
    monkeypatch.setenv("SABER_AMD_SEEDED_WEIGHTS", "1")
    monkeypatch.delenv("SABER_AMD_VIDEO_STORE_GB", raising=False)
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.amg import cfgAMG
    from saber_amd.segmenters.tomo import multiDepthTomoSegmenter
    amg = cfgAMG(npoints=8, crop_n_layers=0, pred_iou_thresh=0.2, stability_score_thresh=0.3, sam2_cfg="small")
    vol = _volume()
    out = {}
    for name, gb in (("off", 0), ("on", 1)):
        seg = multiDepthTomoSegmenter(deviceID=0, cfg=SAM2AdapterConfig(cfg="tiny", amg_cfg=amg, min_mask_area=50, frame_store_gb=gb), min_mask_area=50)
        seg.filter_threshold = -1.0
        vp = seg.adapter._video()
        before = vp.encoded_frames
        out[name] = seg.segment(vol, thickness=2, num_slabs=3, delta_z=2)
        assert seg._prepared is None
        if name == "on":
            assert vp.encoded_frames - before == vol.shape[0] and vp.restored_frames > 0
        else:
            assert vp.encoded_frames - before > vol.shape[0]
        vp.drop_frame_store()
    assert out["off"].shape == vol.shape and out["off"].dtype == np.uint32 and out["off"].max() >= 1
    assert np.array_equal(out["off"], out["on"])
