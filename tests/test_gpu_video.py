"""GPU: the SAM2 video (memory) path, SURVEY.md 8f-1 - kernels against torch formulas, then the tracking loop (add_new_mask,
propagate_in_video both ways, SAM2Adapter.segment_volume with its presence-score filter) against the CPU oracle
(oracle/sam2_video_ref.py) on the reference's own synthetic recipe (saber/adapters/sam3/tests/test_tomogram_predictor.py:67-68,101-104:
default_rng(42).uniform(-1, 1, (Z, 128, 128)) tomogram, centred disk seed of radius min(H, W) // 6)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.op16 import DTYPE, OPS, U, check_bound, from_dev, operand_type, rnd

pytestmark = pytest.mark.gpu


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ck(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()


_ALIVE = []
_ORACLE_FEATS = {}


def _oracle_memo(W):
    """frame content -> oracle features, shared by the oracle predictors built over the SAME weight dict (kept alive here so that its id
    cannot be handed to another dict); every test of this module would otherwise re-encode the same 7 frames on the CPU"""
    return _ORACLE_FEATS.setdefault(id(W), (W, {}))[1]


def dev(t):
    """device copy that outlives the asynchronous launch reading it (a temporary's block is recycled by the caching allocator at once)"""
    _ALIVE.append(t.contiguous().cuda())
    return _ALIVE[-1]


def _rope_and_softmax(lib, op):
    from oracle import sam2_video_ref as V
    g = torch.Generator().manual_seed(0)
    rows, n_rot = 2 * 4096 + 12, 2 * 4096
    x = torch.randn(rows, 256, generator=g)
    cos, sin = V.rope_table(64, 64, 256)
    ref = torch.cat([V.rope_rotate(x[:n_rot].view(2, 4096, 256), cos, sin).reshape(n_rot, 256), x[n_rot:]], 0)
    out = torch.empty(rows, 256, device="cuda")
    outb = torch.empty(rows, 256, dtype=torch.uint16, device="cuda")
    with operand_type(lib, op):
        ck(lib, lib.saber_k_rope(ptr(dev(x)), rows, n_rot, 256, 64, 10000.0, ptr(out), ptr(outb), None))
    torch.cuda.synchronize()
    check_bound(op, "rope fp32 out (abs)", (out.cpu() - ref).abs().max().item(), 2e-4)          # sincosf of angles up to 63 rad
    r64 = ref.double()
    check_bound(op, "rope 16-bit out (abs)", (from_dev(outb, op) - ref).abs().max().item(), 0.03,
                min(0.03 / 8, 3 * U["fp16"] * r64.abs().max().item()), (rnd(r64, "bf16").double() - r64).abs().max().item())
    S = torch.randn(300, 1000, generator=g) * 4
    P = torch.empty(300, 1024, dtype=torch.uint16, device="cuda")
    with operand_type(lib, op):
        ck(lib, lib.saber_k_softmax_rows(ptr(dev(S)), 1000, 300, 1000, 0.0625, ptr(P), 1024, None))
    torch.cuda.synchronize()
    p = from_dev(P, op)
    sref = torch.softmax(S.double() * 0.0625, -1)
    m = sref.max().item()
    # the weights are ~1e-3: the bf16 bound's 2e-5 exceeds a bf16 rounding of them; the fp16 one is one fp16 rounding of the largest
    check_bound(op, "softmax_rows P (abs)", (p[:, :1000].double() - sref).abs().max().item(), 2e-5 + 2 ** -9 * m, U["fp16"] * m,
                (rnd(sref, "bf16").double() - sref).abs().max().item())
    assert (p[:, 1000:] == 0).all()


def test_rope_and_softmax_kernels(gpu_lib):
    _rope_and_softmax(gpu_lib, "bf16")


def test_rope_and_softmax_kernels_fp16(gpu_lib):
    _rope_and_softmax(gpu_lib, "fp16")


def test_conv_and_resize_kernels(gpu_lib):
    g = torch.Generator().manual_seed(1)
    for (H, Cin, Cout) in ((64, 1, 4), (32, 4, 16), (16, 64, 256)):
        x = torch.randn(1, Cin, H, H, generator=g)
        w, b = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.3, torch.randn(Cout, generator=g)
        ref = F.conv2d(x, w, b, stride=2, padding=1)[0].permute(1, 2, 0).reshape(-1, Cout)
        out = torch.empty((H // 2) ** 2, Cout, device="cuda")
        ck(gpu_lib, gpu_lib.saber_k_conv3x3s2(ptr(dev(x[0].permute(1, 2, 0))), H, H, Cin, ptr(dev(w)), ptr(dev(b)), Cout, ptr(out), None))
        assert (out.cpu() - ref).abs().max().item() < 1e-4 * (1 + ref.abs().max().item())
    x = torch.randn(1, 256, 64, 64, generator=g)
    w, b = torch.randn(256, 1, 7, 7, generator=g) * 0.2, torch.randn(256, generator=g)
    ref = F.conv2d(x, w, b, padding=3, groups=256)[0].permute(1, 2, 0).reshape(-1, 256)
    out = torch.empty(4096, 256, device="cuda")
    ck(gpu_lib, gpu_lib.saber_k_dwconv7(ptr(dev(x[0].permute(1, 2, 0))), 64, 64, 256, ptr(dev(w)), ptr(dev(b)), ptr(out), None))
    assert (out.cpu() - ref).abs().max().item() < 1e-4
    m = (torch.rand(1, 1, 1024, 1024, generator=g) > 0.5).float()
    w, b = torch.randn(1, 1, 4, 4, generator=g), torch.randn(1, generator=g)
    out = torch.empty(256, 256, device="cuda")
    ck(gpu_lib, gpu_lib.saber_k_conv4x4s4(ptr(dev(m[0, 0])), 1024, 1024, ptr(dev(w)), ptr(dev(b)), ptr(out), None))
    assert (out.cpu() - F.conv2d(m, w, b, stride=4)[0, 0]).abs().max().item() < 1e-5
    low = F.interpolate(torch.randn(1, 1, 32, 32, generator=g) * 5, size=(256, 256), mode="bicubic")
    for (Ho, aa, post, a, c, fn) in ((1024, 0, 0, 0.0, 0.0, lambda v: v), (1024, 0, 1, 20.0, -10.0, lambda v: torch.sigmoid(v) * 20 - 10),
                                     (600, 0, 3, 2.0, 1.0, lambda v: 2 * v + 1)):
        out = torch.empty(Ho, Ho, device="cuda")
        ck(gpu_lib, gpu_lib.saber_k_resize_plane(ptr(dev(low[0, 0])), 1, 256, 256, ptr(out), Ho, Ho, aa, post, a, c, None))
        ref = fn(F.interpolate(low, size=(Ho, Ho), mode="bilinear", align_corners=False))[0, 0]
        assert (out.cpu() - ref).abs().max().item() < 2e-4, (Ho, post)
    high = m * 20 - 10
    out = torch.empty(256, 256, device="cuda")
    ck(gpu_lib, gpu_lib.saber_k_resize_plane(ptr(dev(high[0, 0])), 1, 1024, 1024, ptr(out), 256, 256, 1, 0, 0.0, 0.0, None))
    ref = F.interpolate(high, size=(256, 256), mode="bilinear", align_corners=False, antialias=True)[0, 0]
    assert (out.cpu() - ref).abs().max().item() < 1e-4
    small = (torch.rand(1, 1, 128, 128, generator=g) > 0.6).float()
    out = torch.empty(1024, 1024, device="cuda")
    ck(gpu_lib, gpu_lib.saber_k_resize_plane(ptr(dev(small[0, 0])), 1, 128, 128, ptr(out), 1024, 1024, 1, 4, 0.5, 0.0, None))
    ref = (F.interpolate(small, size=(1024, 1024), mode="bilinear", align_corners=False, antialias=True) >= 0.5).float()[0, 0]
    assert (out.cpu() != ref).float().mean().item() < 1e-4


@pytest.fixture(scope="module")
def video_case():
    """tiny trunk, seeded weights with a positive object-score bias (the seeded head otherwise predicts 'absent' on every frame and all
    tracked masks collapse to the NO_OBJ constant)"""
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import seeded_weights
    from saber_amd.adapters.sam2.video import VideoPredictor
    cfg = get_config("tiny")
    W = seeded_weights(cfg, 0, video=True)
    W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] = W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] + np.float32(3.0)
    from saber_amd.weights import param_specs
    img_keys = set(param_specs(cfg).keys())
    eng = Engine("tiny", device=0, weights={k: v for k, v in W.items() if k in img_keys}, max_images=3, max_prompts=8)      # windows of 3 frames per encoder pass
    vp = VideoPredictor(eng, W, num_maskmem=2)
    rng = np.random.default_rng(42)
    Z = 7
    tomo = rng.uniform(-1, 1, (Z, 128, 128)).astype(np.float32)
    yy, xx = np.mgrid[:128, :128]
    seed = ((yy - 64) ** 2 + (xx - 64) ** 2 < (128 // 6) ** 2).astype(np.float32)
    yield cfg, W, vp, tomo, seed
    eng.close()


@pytest.fixture(scope="module")
def video_case_f16(video_case):
    """the same model and tomogram on an fp16 handle: what SAM2Adapter._video() builds in production (get_engine -> default_precision()
    "fp16"), so VideoPredictor runs its memory path through _OperandLib with fp16 weight bits and the op16 feature gather"""
    from saber_amd.engine import Engine
    from saber_amd.weights import param_specs
    from saber_amd.adapters.sam2.video import VideoPredictor
    cfg, W, vp, tomo, seed = video_case
    img_keys = set(param_specs(cfg).keys())
    eng = Engine("tiny", device=0, weights={k: v for k, v in W.items() if k in img_keys}, max_images=3, max_prompts=8, precision="fp16")
    vp16 = VideoPredictor(eng, W, num_maskmem=2)
    assert vp16.f16 and vp16.gather_dtype == "op16"
    yield cfg, W, vp16, tomo, seed
    eng.close()


_ORACLE_TRACKS = {}


def _oracle_track(cfg, W, tomo, seed, start):
    """the oracle's tracking run (add_new_mask on `start`, propagation both ways) once per module and case: the bf16 and fp16 legs compare
    against the same CPU run"""
    from oracle import sam2_video_ref as V
    key = (id(W), start, tomo.shape, float(tomo.sum()))
    if key not in _ORACLE_TRACKS:
        ref_frames = V.load_tomogram_frames(tomo)
        P = V.VideoPredictorRef(W, cfg, num_maskmem=2)
        P.feat_memo = _oracle_memo(W)
        P.init_state(ref_frames)
        P.add_new_mask(start, 1, seed)
        ref_out = {}
        for rev in (False, True):
            for t, ids, logits in P.propagate_in_video(start, None, reverse=rev):
                ref_out[(t, rev)] = logits.clone()
        _ORACLE_TRACKS[key] = (W, ref_frames, P, ref_out)
    return _ORACLE_TRACKS[key][1:]


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12)).item()


def _track_compare(cfg, W, vp, tomo, seed, start, bounds):
    """frame by frame: low-res mask logits, object scores and object pointers of the tracked frames, both directions"""
    from oracle import sam2_video_ref as V
    from saber_amd.adapters.sam2.video import load_tomogram_frames
    b_low, b_ptr, b_obj, b_iou = bounds
    frames = load_tomogram_frames(tomo)
    ref_frames, P, ref_out = _oracle_track(cfg, W, tomo, seed, start)
    assert np.abs(frames - ref_frames[:, 0].numpy()).max() < 1e-5
    vp.init_state(frames)
    vp.add_new_mask(start, 1, seed)
    got_out = {}
    for rev in (False, True):
        for t, ids, logits in vp.propagate_in_video(start, None, reverse=rev):
            got_out[(t, rev)] = logits.cpu()
    torch.cuda.synchronize()
    assert set(ref_out) == set(got_out)
    # conditioning frame: the mask itself (+-10 logits through the antialiased down- and the bilinear up-sampling)
    e0 = (got_out[(start, False)] - ref_out[(start, False)]).abs().max().item()
    print("conditioning frame max abs diff", e0)
    assert e0 < 1e-3
    worst = [0.0] * 4
    for t in range(tomo.shape[0]):
        if t == start:
            continue
        r, g = P.out[1]["non_cond"][t], vp.out[1]["non_cond"][t]
        e_low = _rel(g["pred_masks"].cpu(), r["pred_masks"][0, 0])
        e_ptr = _rel(g["obj_ptr"].cpu(), r["obj_ptr"])
        e_obj = abs(g["obj"] - float(r["object_score_logits"]))
        iou = ((got_out[(t, t < start)] > 0) & (ref_out[(t, t < start)] > 0)).sum().item() / max(1, ((got_out[(t, t < start)] > 0) | (ref_out[(t, t < start)] > 0)).sum().item())
        print(f"frame {t}: low-res rel-rms {e_low:.3e}, pointer rel-rms {e_ptr:.3e}, object score |diff| {e_obj:.3e} (ref {float(r['object_score_logits']):.2f}), mask IoU {iou:.4f}")
        worst = [max(worst[0], e_low), max(worst[1], e_ptr), max(worst[2], e_obj), max(worst[3], 1.0 - iou)]
        assert e_low < b_low and e_ptr < b_ptr and e_obj < b_obj and iou > b_iou
    print(f"worst tracked frame ({'fp16' if vp.f16 else 'bf16'} handle): low-res rel-rms {worst[0]:.3e}, pointer rel-rms {worst[1]:.3e}, "
          f"object score |diff| {worst[2]:.3e}, mask IoU {1.0 - worst[3]:.4f}; bounds {bounds}")
    return worst


# low-res logits rel-rms, object pointer rel-rms, object score |diff|, mask IoU of the tracked frames; fp16: measured + 15 %
TRACK_TINY = {"bf16": (2.2e-2, 1.5e-2, 5e-2, 0.995),           # measured <= 1.1e-2 / 7.5e-3 / 2.3e-2 / >= 0.9985
              "fp16": (1.26e-3, 1.08e-3, 2.42e-3, 0.9997)}     # measured 1.09e-3 / 9.4e-4 / 2.11e-3 / 0.9998


def test_fp16_video_bounds_are_below_the_bf16_ones():
    for t in (TRACK_TINY, TRACK_LARGE, VOLUME_TINY):
        for i, (a, b) in enumerate(zip(t["fp16"], t["bf16"])):
            assert (a > b) if (t is VOLUME_TINY and i == 1) or (t is not VOLUME_TINY and i == 3) else (a < b)


def test_tracking_loop_against_oracle(video_case):
    cfg, W, vp, tomo, seed = video_case
    _track_compare(cfg, W, vp, tomo, seed, 3, TRACK_TINY["bf16"])


def test_tracking_loop_against_oracle_fp16(video_case_f16):
    """the production configuration of the video path (fp16 handle, _OperandLib, fp16 weight bits, op16 gather) against the same oracle run"""
    cfg, W, vp, tomo, seed = video_case_f16
    _track_compare(cfg, W, vp, tomo, seed, 3, TRACK_TINY["fp16"])


TRACK_LARGE = {"bf16": (1.2e-2, 1.3e-2, 5.5e-2, 0.997),        # measured <= 5.9e-3 / 6.4e-3 / 2.7e-2 / 1.0000 (4 frames)
               "fp16": (1.39e-3, 9.2e-4, 1.93e-3, 0.9995)}     # measured 1.21e-3 / 8.0e-4 / 1.68e-3 / 1.0000
_LARGE = {}


def _hiera_large_track(precision):
    """The trunk bench.py times on the video path (Hiera-L): 3 frames of 256 x 256 in ONE encoder window, seed on frame 1, forward and
    backward propagation, against oracle/sam2_video_ref.py (the reference drives upstream's video predictor with this trunk for
    `saber segment tomograms`: saber/adapters/sam2/predictor.py:232-348).  The oracle run (~14 s per frame) is shared by both precisions."""
    from saber_amd.adapters.sam2.video import VideoPredictor
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import param_specs, seeded_weights
    if not _LARGE:
        cfg = get_config("large")
        W = seeded_weights(cfg, 0, video=True)
        W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] = W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] + np.float32(3.0)
        rng = np.random.default_rng(42)
        tomo = rng.uniform(-1, 1, (3, 256, 256)).astype(np.float32)
        yy, xx = np.mgrid[:256, :256]
        seed = ((yy - 128) ** 2 + (xx - 128) ** 2 < (256 // 6) ** 2).astype(np.float32)
        _LARGE.update(cfg=cfg, W=W, tomo=tomo, seed=seed)
    cfg, W, tomo, seed = _LARGE["cfg"], _LARGE["W"], _LARGE["tomo"], _LARGE["seed"]
    img_keys = set(param_specs(cfg).keys())
    eng = Engine("large", device=0, weights={k: v for k, v in W.items() if k in img_keys}, max_images=5, max_prompts=8, precision=precision)
    try:
        vp = VideoPredictor(eng, W, num_maskmem=2)
        assert vp.f16 == (precision == "fp16")
        _track_compare(cfg, W, vp, tomo, seed, 1, TRACK_LARGE[precision])
    finally:
        eng.close()


def test_tracking_loop_hiera_large_against_oracle():
    _hiera_large_track("bf16")


def test_tracking_loop_hiera_large_against_oracle_fp16():
    _hiera_large_track("fp16")


_ORACLE_VOLUMES = {}


def _oracle_volume(cfg, W, tomo, seed):
    """the oracle's segment_volume of the tiny case, once per module (both precisions compare against it)"""
    from oracle import sam2_video_ref as V
    if id(W) not in _ORACLE_VOLUMES:
        P = V.VideoPredictorRef(W, cfg, num_maskmem=2)
        P.feat_memo = _oracle_memo(W)
        P.init_state(V.load_tomogram_frames(tomo))
        _ORACLE_VOLUMES[id(W)] = (W, V.segment_volume_ref(P, 3, [seed], tomo.shape, min_presence_score=0.5))
    return _ORACLE_VOLUMES[id(W)][1]


VOLUME_TINY = {"bf16": (0.05, 0.997, 0.02),          # frame scores |diff|, volume IoU, presence |diff|: measured 2.3e-2 / 0.9988 / 7e-3
               "fp16": (7.9e-4, 0.9997, 3.6e-4)}     # measured 6.9e-4 / 0.9998 / 3.1e-4


def test_segment_volume_adapter_against_oracle(video_case):
    """SAM2Adapter.segment_volume end to end: (Z,H,W) uint16, the hook's frame bookkeeping, presence scores from the reference's fit"""
    _segment_volume_compare(video_case, "bf16")


def test_segment_volume_adapter_against_oracle_fp16(video_case_f16):
    _segment_volume_compare(video_case_f16, "fp16")


def _segment_volume_compare(case, precision):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    cfg, W, vp, tomo, seed = case
    b_score, b_iou, b_ps = VOLUME_TINY[precision]
    ref_vol, ref_metrics, ref_scores = _oracle_volume(cfg, W, tomo, seed)
    ad = SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0")
    ad._video_predictor = vp                                         # the fixture's weights (object-score bias) instead of the env-selected ones
    ad.set_volume(tomo)
    vol = ad.segment_volume(3, masks=[seed], min_presence_score=0.5)
    assert vol.shape == tomo.shape and vol.dtype == np.uint16
    print("frame scores (engine):", np.round(ad.frame_scores[:, 0], 3), "\\nframe scores (oracle):", np.round(ref_scores[:, 0], 3))
    assert np.abs(ad.frame_scores - ref_scores).max() < b_score
    assert set(ad.frame_metrics) == set(ref_metrics)
    ps_e = np.array([ad.frame_metrics[z][1]["presence_score"] for z in range(tomo.shape[0])])
    ps_r = np.array([ref_metrics[z][1]["presence_score"] for z in range(tomo.shape[0])])
    print("presence scores:", np.round(ps_e, 3), np.round(ps_r, 3))
    inter = ((vol > 0) & (ref_vol > 0)).sum()
    uni = ((vol > 0) | (ref_vol > 0)).sum()
    print(f"{precision} handle: frame scores max |diff| {np.abs(ad.frame_scores - ref_scores).max():.3e}, volume IoU {inter / max(1, uni):.4f}, "
          f"presence max |diff| {np.abs(ps_e - ps_r).max():.3e}; voxels {int((vol > 0).sum())} vs {int((ref_vol > 0).sum())}; bounds {VOLUME_TINY[precision]}")
    assert (vol[3] == ref_vol[3]).mean() > 0.999                     # the seeded frame
    assert inter / max(1, uni) > b_iou and np.abs(ps_e - ps_r).max() < b_ps
    with pytest.raises(RuntimeError, match="set_volume"):
        SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0").segment_volume(0, [], (3, 8, 8))


def test_adapter_video_path_is_the_fp16_configuration(monkeypatch):
    """what `saber segment tomograms` runs by default: SAM2Adapter._video() on the default environment builds an fp16 handle, and its
    VideoPredictor runs the memory path with fp16 weight bits through _OperandLib and gathers features as op16 - the configuration the
    *_fp16 oracle comparisons above test"""
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    for k in ("SABER_AMD_PRECISION", "SABER_AMD_VIDEO_GATHER"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SABER_AMD_SEEDED_WEIGHTS", "1")
    vp = SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0")._video()
    assert vp.f16 is True and vp.gather_dtype == "op16" and vp.eng.operands == "fp16"


def test_reference_script_assertions_shape_dtype_and_reset(video_case):
    """What the reference's own adapter test script asserts (saber/adapters/sam3/tests/test_tomogram_predictor.py:75-81,139-142,150-169,
    written for the SAM3 adapter against the same BaseAdapter contract): the loaded state counts Z frames, segment_volume returns
    (Z,H,W) uint16, reset_state clears the prompts."""
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    cfg, W, vp, tomo, seed = video_case
    ad = SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0")
    ad._video_predictor = vp
    ad.set_volume(tomo)
    assert ad.inference_state.num_frames == tomo.shape[0] and tuple(ad.inference_state.images.shape) == (tomo.shape[0], 1024, 1024)
    vol = ad.segment_volume(3, masks=[seed], max_frame_num_to_track=2, min_presence_score=0.0)
    assert vol.shape == tomo.shape and vol.dtype == np.uint16
    assert not vol[0].any() and not vol[6].any()                 # max_frame_num_to_track = 2: frames 1..5 only
    ad.add_new_mask(frame_idx=0, obj_id=99, mask=np.ones((128, 128), dtype=np.float32) * 0.5)
    assert 99 in ad.inference_state.obj_ids
    ad.reset_state()
    assert len(ad.inference_state.obj_ids) == 0 and not ad.inference_state.out
    st = ad.inference_state                                      # an object without any prompt: upstream's preflight error
    st.obj_ids.append(1); st.out[1] = {"cond": {}, "non_cond": {}}; st.temp[1] = {}
    with pytest.raises(RuntimeError, match="No input points or masks"):
        list(ad.propagate_in_video(0))
    ad.reset_state()


def test_add_new_points_single_click_against_oracle(video_case):
    """add_new_points_or_box with one positive click on an untracked frame (initial conditioning frame: SAM heads on the frame's own
    features, multimask, best IoU), then two tracked frames, against the oracle; on a handle without the exact precision mode boxes /
    several clicks raise NotImplementedError (test_box_and_several_clicks_against_oracle runs them)."""
    from oracle import sam2_video_ref as V
    from saber_amd.adapters.sam2.video import load_tomogram_frames
    cfg, W, vp, tomo, seed = video_case
    frames = load_tomogram_frames(tomo)
    P = V.VideoPredictorRef(W, cfg, num_maskmem=2)
    P.feat_memo = _oracle_memo(W)
    P.init_state(V.load_tomogram_frames(tomo), video_hw=(1024, 1024))
    vp.init_state(frames, video_hw=(1024, 1024))
    click, lab = np.array([[512.0, 500.0]], np.float32), np.array([1], np.int32)
    _, ids_r, vr = P.add_new_points_or_box(3, 1, points=click, labels=lab)
    _, ids_e, ve = vp.add_new_points_or_box(3, 1, points=click, labels=lab)
    assert ids_r == ids_e == [1] and tuple(ve.shape) == (1, 1, 1024, 1024)
    e0 = _rel(vp.temp[1][3]["pred_masks"].cpu(), P.temp[1][3]["pred_masks"][0, 0])
    ep = _rel(vp.temp[1][3]["obj_ptr"].cpu(), P.temp[1][3]["obj_ptr"])
    print("click frame: low-res rel-rms", e0, "pointer", ep)
    assert e0 < 2.2e-2 and ep < 1.4e-2
    ref = {t: lg for t, _, lg in P.propagate_in_video(3, max_frame_num_to_track=2)}
    got = {t: lg for t, _, lg in vp.propagate_in_video(3, max_frame_num_to_track=2)}
    assert sorted(ref) == sorted(got) == [3, 4, 5]
    for t in ref:
        g, r = got[t][0, 0].cpu() > 0, ref[t][0, 0] > 0
        iou = float((g & r).sum()) / max(1.0, float((g | r).sum()))
        print("frame", t, "mask IoU", iou)
        assert iou > 0.97 or (not g.any() and not r.any())        # seeded weights: logits of a raw SAM output hover near zero over much of the frame (measured 0.983-0.99)
    with pytest.raises(NotImplementedError):
        vp.add_new_points_or_box(0, 2, box=[10, 10, 50, 50])
    with pytest.raises(NotImplementedError):
        vp.add_new_points_or_box(0, 2, points=[[1, 1], [2, 2]], labels=[1, 1])
    with pytest.raises(ValueError):
        vp.add_new_points_or_box(0, 2, points=[[1, 1]])
    vp.reset_state()


def test_box_and_several_clicks_against_oracle():
    """add_new_points_or_box with a box, a box + a click, and clicks accumulated over two calls (clear_old_points=False), on an untracked
    frame: the oracle's restatement of upstream's point handling (box corners as labels 2 / 3 in front, single-mask output beyond one point)
    against the product, whose engine decodes such prompts in its exact precision mode (the handle is created with precision="exact" and
    runs everything else - encoder, tracked frames - in bf16); then two tracked frames."""
    from oracle import sam2_video_ref as V
    from saber_amd.adapters.sam2.video import VideoPredictor, load_tomogram_frames
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import param_specs, seeded_weights
    cfg = get_config("tiny")
    W = seeded_weights(cfg, 0, video=True)
    W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] = W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] + np.float32(3.0)
    img_keys = set(param_specs(cfg).keys())
    eng = Engine("tiny", device=0, weights={k: v for k, v in W.items() if k in img_keys}, max_images=3, max_prompts=8, precision="exact")
    eng.set_precision("bf16")
    try:
        vp = VideoPredictor(eng, W, num_maskmem=2)
        rng = np.random.default_rng(5)
        tomo = rng.uniform(-1, 1, (5, 128, 128)).astype(np.float32)
        P = V.VideoPredictorRef(W, cfg, num_maskmem=2)
        P.feat_memo = _oracle_memo(W)
        for case in ("box+click", "two calls"):          # (a box alone: tests/test_gpu_exact.py at the decoder level)
            P.init_state(V.load_tomogram_frames(tomo), video_hw=(1024, 1024))
            vp.init_state(load_tomogram_frames(tomo), video_hw=(1024, 1024))
            for pred in (P, vp):
                if case == "box":
                    out = pred.add_new_points_or_box(1, 7, box=[300.0, 280.0, 720.0, 700.0])
                elif case == "box+click":
                    out = pred.add_new_points_or_box(1, 7, points=[[500.0, 480.0]], labels=[1], box=[300.0, 280.0, 720.0, 700.0])
                else:
                    pred.add_new_points_or_box(1, 7, points=[[500.0, 480.0]], labels=[1])
                    out = pred.add_new_points_or_box(1, 7, points=[[650.0, 300.0]], labels=[0], clear_old_points=False)
                assert out[1] == [7] and tuple(out[2].shape) == (1, 1, 1024, 1024)
            assert eng.precision == "bf16"                                  # restored after the exact-mode decode
            e0 = _rel(vp.temp[7][1]["pred_masks"].cpu(), P.temp[7][1]["pred_masks"][0, 0])
            ep = _rel(vp.temp[7][1]["obj_ptr"].cpu(), P.temp[7][1]["obj_ptr"])
            print(f"{case}: prompted frame low-res rel-rms {e0:.3e}, pointer {ep:.3e}")
            assert e0 < 2.2e-2 and ep < 1.4e-2                              # (the frame's features come from the bf16 encoder: the bounds of the single-click test)
            n_track = 2 if case == "box+click" else 1          # (the second case repeats the tracking chain of the first: one frame is enough)
            ref = {t: lg for t, _, lg in P.propagate_in_video(1, max_frame_num_to_track=n_track)}
            got = {t: lg for t, _, lg in vp.propagate_in_video(1, max_frame_num_to_track=n_track)}
            assert sorted(ref) == sorted(got) == list(range(1, 2 + n_track))
            for t in ref:
                g, r = got[t][0, 0].cpu() > 0, ref[t][0, 0] > 0
                iou = float((g & r).sum()) / max(1.0, float((g | r).sum()))
                print(f"{case}: frame {t} mask IoU {iou:.4f}")
                assert iou > 0.97 or (not g.any() and not r.any())
        with pytest.raises(ValueError):
            vp.add_new_points_or_box(0, 9, box=[1, 1, 5, 5], clear_old_points=False)
        # ---- corrections of a frame that a propagation has already gone over (upstream: is_init_cond_frame False): memory-conditioned
        # features in the direction the frame was tracked, previous output as the mask prompt, the result stays a non-conditioning output
        yy, xx = np.mgrid[:128, :128]
        seed = ((yy - 64) ** 2 + (xx - 64) ** 2 < (128 // 6) ** 2).astype(np.float32)
        P.init_state(V.load_tomogram_frames(tomo), video_hw=(1024, 1024))
        vp.init_state(load_tomogram_frames(tomo), video_hw=(1024, 1024))
        for pred in (P, vp):
            pred.add_new_mask(1, 1, seed)
            for _ in pred.propagate_in_video(1, max_frame_num_to_track=3):
                pass
        for step, kw in (("one click (bf16 decoder, multimask)", dict(points=[[600.0, 500.0]], labels=[0])),
                         ("second click (exact-mode decoder, single mask)", dict(points=[[420.0, 430.0]], labels=[1], clear_old_points=False))):
            r = P.add_new_points_or_box(3, 1, **kw)
            g = vp.add_new_points_or_box(3, 1, **kw)
            e0 = _rel(vp.temp[1][3]["pred_masks"].cpu(), P.temp[1][3]["pred_masks"][0, 0])
            ep = _rel(vp.temp[1][3]["obj_ptr"].cpu(), P.temp[1][3]["obj_ptr"])
            gi, ri = g[2][0, 0].cpu() > 0, r[2][0, 0] > 0
            iou = float((gi & ri).sum()) / max(1.0, float((gi | ri).sum()))
            print(f"correction of tracked frame 3, {step}: low-res rel-rms {e0:.3e}, pointer {ep:.3e}, returned mask IoU {iou:.4f}")
            assert e0 < 3e-2 and ep < 2e-2 and (iou > 0.97 or (not gi.any() and not ri.any()))
            assert vp.temp[1][3]["is_cond"] is False and P.temp[1][3]["is_cond"] is False
        ref = {t: lg for t, _, lg in P.propagate_in_video(4, max_frame_num_to_track=0)}        # preflight: frame 3's corrected output + its memory replace the tracked one
        got = {t: lg for t, _, lg in vp.propagate_in_video(4, max_frame_num_to_track=0)}
        assert 3 in vp.out[1]["non_cond"] and 3 not in vp.out[1]["cond"] and sorted(ref) == sorted(got) == [4]
        g4, r4 = got[4][0, 0].cpu() > 0, ref[4][0, 0] > 0
        iou = float((g4 & r4).sum()) / max(1.0, float((g4 | r4).sum()))
        print(f"frame 4 re-tracked on the corrected memory of frame 3: mask IoU {iou:.4f}")
        assert iou > 0.97 or (not g4.any() and not r4.any())
    finally:
        eng.close()


def test_two_objects_segment_volume_against_oracle(video_case):
    """two seed masks (two objects tracked independently, later object ids overwrite earlier ones where they overlap, the backward pass
    fills only frames the forward pass left empty): SAM2Adapter.segment_volume against the oracle's, label by label"""
    from oracle import sam2_video_ref as V
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    cfg, W, vp, tomo, seed = video_case
    yy, xx = np.mgrid[:128, :128]
    seed2 = ((yy - 40) ** 2 + (xx - 90) ** 2 < 14 ** 2).astype(np.float32)
    P = V.VideoPredictorRef(W, cfg, num_maskmem=2)
    P.feat_memo = _oracle_memo(W)
    P.init_state(V.load_tomogram_frames(tomo))
    ref_vol, ref_metrics, ref_scores = V.segment_volume_ref(P, 2, [seed, seed2], tomo.shape, min_presence_score=0.0)
    ad = SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0")
    ad._video_predictor = vp
    ad.set_volume(tomo)
    vol = ad.segment_volume(2, masks=[seed, seed2], min_presence_score=0.0)
    assert vol.shape == tomo.shape and vol.dtype == np.uint16 and set(np.unique(vol)) <= {0, 1, 2}
    assert ad.frame_scores.shape == ref_scores.shape == (tomo.shape[0], 2)
    assert np.abs(ad.frame_scores - ref_scores).max() < 0.06
    for lab in (1, 2):
        inter = ((vol == lab) & (ref_vol == lab)).sum()
        uni = ((vol == lab) | (ref_vol == lab)).sum()
        print(f"object {lab}: volume IoU {inter / max(1, uni):.4f} ({int((vol == lab).sum())} vs {int((ref_vol == lab).sum())} voxels)")
        # object 1 survives only where object 2's (image-filling, seeded-weights) mask is absent: ~1 400 voxels whose outline is object 2's
        # near-zero-logit boundary, so a few dozen voxels flip with the bf16 residual (measured 0.967); the large label is tight
        assert inter / max(1, uni) > (0.995 if uni > 50000 else 0.94)


def test_window_encodes_sharded_over_ranks(tmp_path):
    """SURVEY.md 8e (propagation path): the per-frame Hiera passes of a window shard over the ranks of the process group and are
    all-gathered (saber_export_slots / saber_import_slots); the replicated tracking chain must then give every rank exactly what one
    process gives.  Two gloo ranks on this one GPU (RCCL needs a GPU per rank), 7 frames in windows of 3: shares of 2 + 1 frames and a
    last window whose second rank has nothing to encode."""
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "video_shard_worker.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    base = str(tmp_path / "one.npz")
    subprocess.run([sys.executable, worker, base], check=True, env=env, timeout=300)
    procs = []
    for r in range(2):
        e = dict(env, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
        procs.append(subprocess.Popen([sys.executable, worker, str(tmp_path / f"r{r}.npz")], env=e))
    for p in procs:
        assert p.wait(timeout=300) == 0
    one = np.load(base)
    assert int(one["sharded"]) == 1 and (one["vol"] > 0).sum() > 0
    for r in range(2):
        got = np.load(str(tmp_path / f"r{r}.npz"))
        assert int(got["sharded"]) == 2
        assert np.array_equal(got["vol"], one["vol"]) and np.array_equal(got["scores"], one["scores"]), r


def test_window_encodes_sharded_with_16_bit_gather(tmp_path):
    """SABER_AMD_VIDEO_GATHER=op16: the sharded window encodes ship their features as 16-bit (8 MiB per frame instead of 16).  Every rank
    decodes from the same rounded features, so the two ranks agree bit for bit; against the unsharded run the volume differs by the rounding
    of the features only."""
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "video_shard_worker.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    base = str(tmp_path / "one.npz")
    subprocess.run([sys.executable, worker, base], check=True, env=env, timeout=300)
    procs = []
    for r in range(2):
        e = dict(env, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT="29537", SABER_AMD_VIDEO_GATHER="op16")
        procs.append(subprocess.Popen([sys.executable, worker, str(tmp_path / f"h{r}.npz")], env=e))
    for p in procs:
        assert p.wait(timeout=300) == 0
    one, g0, g1 = np.load(base), np.load(str(tmp_path / "h0.npz")), np.load(str(tmp_path / "h1.npz"))
    assert int(g0["sharded"]) == 2 and int(g1["sharded"]) == 2
    assert np.array_equal(g0["vol"], g1["vol"]) and np.array_equal(g0["scores"], g1["scores"])
    a, b = g0["vol"] > 0, one["vol"] > 0
    iou = (a & b).sum() / max(1, (a | b).sum())
    print("16-bit gather vs unsharded: volume IoU", iou, "max |score diff|", np.abs(g0["scores"] - one["scores"]).max())
    assert iou > 0.99 and np.abs(g0["scores"] - one["scores"]).max() < 0.1


def test_frames_larger_than_1024_px_on_the_device(gpu_lib):
    """load_tomogram_frames_device on a tomogram above the model's resolution (Gaussian anti-aliasing as skimage's down-sampling resize
    applies it, saber/adapters/preprocessing.py:21) against the oracle's scipy restatement; mixed case: one axis down-, one up-sampled."""
    from oracle import sam2_video_ref as V
    from saber_amd.adapters.sam2.video import load_tomogram_frames_device
    rng = np.random.default_rng(5)
    for shape in ((2, 1536, 1300), (1, 2048, 2048), (2, 1100, 700)):
        tomo = rng.normal(0, 1, shape).astype(np.float32)
        ref = V.load_tomogram_frames(tomo)[:, 0]
        got = load_tomogram_frames_device(tomo, gpu_lib, torch.device("cuda:0"))
        torch.cuda.synchronize()
        err = (got.cpu() - ref).abs().max().item()
        print(shape, "frames max abs diff", err)
        assert got.shape == (shape[0], 1024, 1024) and err < 2e-5


def _flash256(lib, op, cases, qk_scale=1.0):
    """csrc/flash256.hip against fp64: one head of 256 channels, with and without the split over the keys"""
    g = torch.Generator().manual_seed(3)
    T = DTYPE[op]
    for n_q, n_keys in cases:
        Q = (torch.randn(n_q, 256, generator=g) * 0.7 * qk_scale).to(T)
        K = (torch.randn(n_keys, 256, generator=g) * 0.7 * qk_scale).to(T)
        V = torch.randn(n_keys, 256, generator=g).to(T)
        bv = torch.randn(256, generator=g)
        S = (Q.cuda().double() @ K.cuda().double().T) * 0.0625
        ref = torch.softmax(S, -1) @ V.cuda().double() + bv.cuda().double()
        keep = torch.ones(n_q, dtype=torch.bool, device="cuda")
        if qk_scale != 1.0:
            # scores of order 1e4 .. 1e6: the fp32 scores' absolute error grows with them; queries whose two largest scaled scores lie within
            # a few units move with the accumulation order (not the type) and are left out
            top = S.topk(2, dim=-1).values
            keep = top[:, 0] - top[:, 1] > 20.0
            print(f"largest |q . k| before the scale {(S.abs().max().item() / 0.0625):.2e}; queries with a clear maximum {keep.float().mean().item():.4f}")
            assert keep.float().mean().item() > 0.95
        out = torch.empty(n_q, 256, dtype=torch.uint16, device="cuda")
        ws = torch.empty((n_q // 64) * 8 * 64 * 258, device="cuda")
        for w in (ws, None):
            with operand_type(lib, op):
                ck(lib, lib.saber_k_flash256(ptr(dev(Q.view(torch.uint16))), ptr(dev(K.view(torch.uint16))), ptr(dev(V.view(torch.uint16))), n_q, n_keys, 0.0625,
                                             ptr(dev(bv)), ptr(out), ptr(w), 0 if w is None else w.numel(), None))
            torch.cuda.synchronize()
            got = out.view(T).double()
            assert torch.isfinite(got).all()
            r = ref[keep]
            check_bound(op, f"flash256 n_q={n_q} n_keys={n_keys} split={'yes' if w is not None else 'no'} max abs", (got[keep] - r).abs().max().item(),
                        0.03, min(0.03 / 8, 3 * U["fp16"] * r.abs().max().item()), (rnd(r, "bf16").double() - r).abs().max().item())   # 16-bit P and output


FLASH_CASES = ((4096, 4096), (4096, 8212), (128, 100), (64, 31))


def test_flash256_attention_kernel(gpu_lib):
    """key counts that are and are not multiples of the 64-key blocks (the memory bank: 2 x 4096 spatial tokens + 4 tokens per object
    pointer), with and without the split over the keys"""
    _flash256(gpu_lib, "bf16", FLASH_CASES)


def test_flash256_attention_kernel_fp16(gpu_lib):
    _flash256(gpu_lib, "fp16", FLASH_CASES)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("qk_scale", [60.0, 150.0])
def test_flash256_large_scores(gpu_lib, qk_scale, op):
    """Q and K scaled so that the scores before the scale are of order 1e4 .. 1e6 (operands and outputs within fp16's range): an intermediate
    kept in the 16-bit type would overflow in fp16 where bf16's range hides it"""
    _flash256(gpu_lib, op, ((512, 1000), (64, 8212)), qk_scale)
