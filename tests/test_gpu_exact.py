"""GPU: the engine's EXACT-precision mode (saber_engine_set_precision, csrc/exact.hip) against the fp32 CPU oracle at the north star's
tolerance: float logits within 1e-3 rel, |IoU - 1| < 1e-3 (BASELINE.json north_star; the reference runs fp32: saber/utils/io.py:127-132).

The bf16 production path sits 3-8e-3 from the fp32 oracle (tests/test_gpu_engine.py); these tests show (a) a mode of the SAME engine (same
token order, slots, weights, AMG driver, C-ABI) that meets 1e-3 exists, (b) what bf16 costs relative to it on the same handle, and - since
the exact mode executes the UNFOLDED decoder composition and the exact-erf GELU - (c) that the production kernels' folded t2i / i2t algebra,
fused upscaling and fitted GELU agree with an independent formulation up to their operand rounding.
"""
import os

import numpy as np
import pytest
import torch

from saber_amd.utils import npz_parts

pytestmark = pytest.mark.gpu

TOL = 1e-3        # north star: "float logits within 1e-3 rel"


def rel_rms(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12)).item()


def rel_max(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


@pytest.fixture(scope="module")
def engine_exact(large_weights):
    from saber_amd.engine import Engine
    cfg, W = large_weights
    eng = Engine("large", device=0, weights=W, max_images=2, max_prompts=32, precision="exact")
    yield eng
    eng.close()


def test_exact_encoder_within_1e3_of_fp32_oracle(engine_exact, image, oracle_feats):
    engine_exact.set_precision("exact")
    engine_exact.encode(torch.from_numpy(image).cuda())
    got = engine_exact.get_features(0)
    torch.cuda.synchronize()
    errs = {k: (rel_rms(got[k].cpu(), oracle_feats[k][0]), rel_max(got[k].cpu(), oracle_feats[k][0])) for k in ("image_embed", "feat_s0", "feat_s1")}
    print("EXACT encoder vs fp32 oracle (rel-rms, max-abs / max):", errs)
    for k, (rms, mx) in errs.items():
        assert rms < TOL and mx < TOL, (k, rms, mx)


def test_exact_decoder_and_m2m_within_1e3(engine_exact, image, oracle_large, oracle_feats):
    from oracle import sam2_ref
    cfg, W = oracle_large
    engine_exact.set_precision("exact")
    engine_exact.encode(torch.from_numpy(image).cuda())
    rng = np.random.default_rng(3)
    pts = torch.tensor(rng.uniform(0, 1024, (8, 2)).astype(np.float32))
    lab = torch.ones(8, 1, dtype=torch.int64)
    low, iou, obj = engine_exact.decode_points(pts.cuda(), slot=0, multimask=True)
    torch.cuda.synchronize()
    with torch.no_grad():
        sp, de = sam2_ref.prompt_encoder(W, pts[:, None], lab, None)
        o_low, o_iou, o_obj, _, _ = sam2_ref.mask_decoder(W, oracle_feats, sp, de, True)
    e_low, m_low = rel_rms(low.cpu(), o_low), rel_max(low.cpu(), o_low)
    e_iou = (iou.cpu() - o_iou).abs().max().item()
    e_obj = ((obj.cpu() - o_obj[:, 0]).abs().max() / o_obj.abs().max()).item()
    print(f"EXACT end to end vs fp32 oracle: low-res logits rel-rms {e_low:.2e} (max {m_low:.2e}), iou abs {e_iou:.2e}, obj rel {e_obj:.2e}")
    assert e_low < TOL and m_low < TOL and e_iou < TOL and e_obj < TOL
    # thresholded masks: |IoU - 1| per mask
    a, b = (low.cpu() > 0).flatten(2), (o_low > 0).flatten(2)
    inter, uni = (a & b).sum(-1).double(), (a | b).sum(-1).double()
    miou = torch.where(uni > 0, inter / uni.clamp(min=1), torch.ones_like(uni))
    print("EXACT per-mask |IoU - 1|: median", (1 - miou).median().item(), "max", (1 - miou).max().item())
    assert (1 - miou).max().item() < TOL
    # m2m pass: mask prompt + dynamic single-mask selection, on the oracle's own first-pass logits
    mi = torch.clamp(o_low[:, 0], -32, 32).contiguous()
    low2, iou2, _ = engine_exact.decode_points(pts.cuda(), slot=0, multimask=False, mask_input=mi.cuda())
    with torch.no_grad():
        sp, de = sam2_ref.prompt_encoder(W, pts[:, None], lab, mi[:, None])
        r_low2, r_iou2, _, _, _ = sam2_ref.mask_decoder(W, oracle_feats, sp, de, False)
    e2, m2 = rel_rms(low2.cpu(), r_low2), rel_max(low2.cpu(), r_low2)
    print(f"EXACT m2m vs fp32 oracle: low-res rel-rms {e2:.2e} (max {m2:.2e}), iou abs {(iou2.cpu() - r_iou2).abs().max().item():.2e}")
    assert e2 < TOL and m2 < TOL and (iou2.cpu() - r_iou2).abs().max().item() < TOL


def test_price_of_bf16_on_the_same_handle(engine_exact, image):
    """The same handle, the same calls, the two precisions: what the bf16 operands cost (reported; bounded at 2x the values measured
    against the oracle in tests/test_gpu_engine.py) - and an independent check of the production decoder kernels (folded projections,
    fused upscaling, fitted GELU) against the unfolded fp32 composition on IDENTICAL features."""
    rng = np.random.default_rng(5)
    pts = torch.tensor(rng.uniform(0, 1024, (16, 2)).astype(np.float32)).cuda()
    img = torch.from_numpy(image).cuda()
    engine_exact.set_precision("exact")
    engine_exact.encode(img)
    fx = {k: v.clone() for k, v in engine_exact.get_features(0).items()}
    lx, ix, ox = engine_exact.decode_points(pts, slot=0, multimask=True)
    engine_exact.set_precision("bf16")
    lb_same, ib_same, _ = engine_exact.decode_points(pts, slot=0, multimask=True)        # bf16 decoder on the EXACT features
    engine_exact.encode(img)
    fb = engine_exact.get_features(0)
    lb, ib, ob = engine_exact.decode_points(pts, slot=0, multimask=True)
    torch.cuda.synchronize()
    engine_exact.set_precision("exact")
    enc = {k: rel_rms(fb[k], fx[k]) for k in fx}
    d_same, d_e2e = rel_rms(lb_same, lx), rel_rms(lb, lx)
    print("price of bf16, encoder features (rel-rms bf16 vs exact):", enc)
    print(f"price of bf16, decoder alone on identical features: low-res {d_same:.2e}, iou abs {(ib_same - ix).abs().max().item():.2e}; end to end: low-res {d_e2e:.2e}")
    assert enc["image_embed"] < 1.2e-2 and enc["feat_s1"] < 8.4e-3 and enc["feat_s0"] < 5.6e-3
    assert d_same < 1.1e-2 and d_e2e < 1.6e-2
    assert ((lb_same > 0) == (lx > 0)).float().mean().item() > 0.997


def test_exact_config1_tiny_golden():
    """BASELINE configs[0] (512^2 micrograph, Hiera-tiny: the padded 14 x 14 / 7 x 7 window layout, head dim 96) against the HF-validated
    golden, at 1e-3."""
    from oracle.make_golden_model import config1_image
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import seeded_weights
    M = np.load(os.path.join(os.path.dirname(__file__), "golden", "sam2_tiny_seed0.npz"))
    eng = Engine("tiny", device=0, weights=seeded_weights(get_config("tiny"), 0), max_images=1, max_prompts=8, precision="exact")
    try:
        eng.encode(torch.from_numpy(config1_image()).cuda())
        f = eng.get_features(0)
        pts = torch.tensor([[512.0, 512.0]])
        low, iou, obj = eng.decode_points(pts.cuda(), slot=0, multimask=True)
        torch.cuda.synchronize()
        g = {"image_embed": f["image_embed"][::8, ::4, ::4], "feat_s0": f["feat_s0"][::4, ::16, ::16], "feat_s1": f["feat_s1"][::8, ::8, ::8]}
        errs = {k: rel_rms(g[k].cpu(), torch.from_numpy(M[k + "_sub"])) for k in g}
        e_low = rel_rms(low[0, :, ::4, ::4].cpu(), torch.from_numpy(M["low_res_sub"]))
        e_iou = float(np.abs(iou.cpu().numpy() - M["iou"]).max())
        print("EXACT config 1 (tiny) vs golden:", errs, "low-res", e_low, "iou", e_iou)
        assert max(errs.values()) < TOL and e_low < TOL and e_iou < TOL
        mi = torch.clamp(low[:, 0], -32, 32).contiguous()
        low2, iou2, _ = eng.decode_points(pts.cuda(), slot=0, multimask=False, mask_input=mi)
        e2 = rel_rms(low2[0, :, ::4, ::4].cpu(), torch.from_numpy(M["m2m_low_res_sub"]))
        print("EXACT config 1 m2m low-res", e2)
        assert e2 < TOL
    finally:
        eng.close()


@pytest.mark.parametrize("trunk", ["small", "base"])
def test_exact_other_trunks(trunk, image):
    from oracle import sam2_ref
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import seeded_weights
    cfg = get_config(trunk)
    Wnp = seeded_weights(cfg, 1)
    W = sam2_ref.to_torch(Wnp)
    eng = Engine(trunk, device=0, weights=Wnp, max_images=2, max_prompts=8, precision="exact")
    try:
        with torch.no_grad():
            feats = sam2_ref.encode_image(W, cfg, sam2_ref.sam2_transforms(np.repeat(image[..., None], 3, 2)))
        eng.encode(torch.from_numpy(image).cuda(), [[0, 0, 512, 512], [0, 0, 1024, 1024]], slot0=0)
        got = eng.get_features(1)
        errs = {k: rel_rms(got[k].cpu(), feats[k][0]) for k in ("image_embed", "feat_s0", "feat_s1")}
        print(trunk, "EXACT encoder rel-rms:", errs)
        assert max(errs.values()) < TOL
    finally:
        eng.close()


def test_exact_default_grid_amg_golden(large_weights):
    """BASELINE configs[1] at cfgAMG's default grid and crop pyramid (21 crops, 3 072 grid prompts + 9 216 m2m refinements) in exact mode
    against the fp32 oracle's committed result (tests/golden/amg_default_grid_seed0.npz): the SAME mask count (227) and per-mask
    |IoU - 1| <= 1e-3 in the median."""
    from oracle import saber_ref
    from saber_amd.engine import Engine, make_amg_params, unpack_bits
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "amg_default_grid_seed0.npz"))
    cfg, W = large_weights
    eng = Engine("large", device=0, weights=W, max_images=21, max_prompts=1024, precision="exact")
    try:
        img = eng.prepare(torch.from_numpy(saber_ref.synthetic_slice(seed=0)).cuda())
        amg = dict(npoints=32, crop_n_layers=2, pred_iou_thresh=0.8055, stability_score_thresh=0.0, box_nms_thresh=1.0, crop_nms_thresh=1.0)
        import time
        t0 = time.time()
        bits, meta = eng.amg_generate(img, make_amg_params(amg), max_masks=4096)
        torch.cuda.synchronize()
        print(f"EXACT default-grid AMG: {time.time() - t0:.1f} s")
        got = unpack_bits(bits, 1024)[:, 2::4, 2::4]
        ref = np.unpackbits(G["quarter_bits"], axis=-1).astype(bool)
        n_ref, n_got = int(G["count"]), len(meta)
        gf = got.reshape(n_got, -1).astype(np.float32)
        rf = ref.reshape(n_ref, -1).astype(np.float32)
        inter = rf @ gf.T
        uni = rf.sum(1)[:, None] + gf.sum(1)[None] - inter
        best = (inter / np.maximum(uni, 1)).max(1)
        dev = 1.0 - best
        print(f"EXACT default-grid AMG: oracle {n_ref} masks, engine {n_got}; per-mask |IoU - 1| median {np.median(dev):.2e}, p90 {np.quantile(dev, 0.9):.2e}, max {dev.max():.2e}")
        # predicted IoUs of the matched masks
        order = (inter / np.maximum(uni, 1)).argmax(1)
        piou = np.array([meta[j].predicted_iou for j in order])
        print("predicted_iou abs diff of matched masks: max", np.abs(piou - G["predicted_iou"]).max())
        assert n_got == n_ref, (n_got, n_ref)
        assert np.median(dev) <= TOL
        assert np.abs(piou - G["predicted_iou"]).max() < TOL
    finally:
        eng.close()


def _amg_vs_golden(eng, name, amg):
    from oracle import saber_ref
    from saber_amd.engine import make_amg_params, unpack_bits
    G = npz_parts.load(os.path.join(os.path.dirname(__file__), "golden", name))
    img = eng.prepare(torch.from_numpy(saber_ref.synthetic_slice(seed=0)).cuda())
    bits, meta = eng.amg_generate(img, make_amg_params(amg), max_masks=4096)
    torch.cuda.synchronize()
    got = unpack_bits(bits, 1024)[:, 2::4, 2::4] if len(meta) else np.zeros((0, 256, 256), dtype=bool)
    ref = np.unpackbits(G["quarter_bits"], axis=-1).astype(bool)
    return G, meta, got, ref


def test_exact_default_grid_filters_goldens(large_weights):
    """The generator's FILTERS at the default grid against the fp32 oracle (what the seeded weights allow: DESIGN.md section 3).
    (a) stability_score_thresh and pred_iou_thresh at the candidates' medians, NMS off: each score filter removes about half, the survivors and
    their ORDER must be the oracle's; (b) cfgAMG's own stability 0.92 / box NMS 0.7 / crop NMS 0.7 with pred_iou_thresh 0: per-crop NMS and the
    cross-crop NMS (score 1 / crop area) leave one mask - the same one."""
    from saber_amd.engine import Engine
    cfg, W = large_weights
    gold = os.path.join(os.path.dirname(__file__), "golden")
    if not (npz_parts.exists(os.path.join(gold, "amg_default_grid_stability_seed0.npz")) and npz_parts.exists(os.path.join(gold, "amg_default_grid_cfgamg_seed0.npz"))):
        pytest.skip("filters goldens not generated (python -m oracle.make_golden_amg with VARIANT=stability / cfgamg: ~40 min of CPU each)")
    eng = Engine("large", device=0, weights=W, max_images=21, max_prompts=1024, precision="exact")
    try:
        # (a) the two score filters
        G, meta, got, ref = _amg_vs_golden(eng, "amg_default_grid_stability_seed0.npz",
                                           dict(npoints=32, crop_n_layers=2, pred_iou_thresh=0.7459, stability_score_thresh=0.9071, box_nms_thresh=1.0, crop_nms_thresh=1.0))
        n_ref, n_got = int(G["count"]), len(meta)
        # Candidates are identified by (point, crop box, area rank): every oracle survivor must be among the engine's, in the oracle's ORDER.  A
        # candidate whose stability score (a ratio of two pixel counts) or predicted IoU sits ON a threshold - both thresholds are the medians of
        # their distributions - may fall on either side of it by one float ulp: such extras / misses are allowed only within 1e-5 of a threshold.
        def key(pt, cb):
            return tuple(np.round(np.concatenate([np.asarray(pt, dtype=np.float64), np.asarray(cb, dtype=np.float64)]), 2))
        eng_keys = [key(m.point_xy, m.crop_box_xywh) for m in meta]
        ref_keys = [key(G["point"][i], G["crop_box"][i]) for i in range(n_ref)]
        # (three m2m candidates share a point: disambiguate by order of appearance)
        from collections import defaultdict
        pos = defaultdict(list)
        for j, k in enumerate(eng_keys):
            pos[k].append(j)
        match, used = [], set()
        for i, k in enumerate(ref_keys):
            # the (up to three) m2m candidates of one point are told apart by their predicted IoU
            bi, bd = -1, 1e-4
            for j in pos.get(k, []):
                d = abs(meta[j].predicted_iou - float(G["predicted_iou"][i]))
                if j not in used and d < bd:
                    bi, bd = j, d
            best = (got[bi] & ref[i]).sum() / max(1, (got[bi] | ref[i]).sum()) if bi >= 0 else -1.0
            match.append((bi, best))
            if bi >= 0:
                used.add(bi)
        missing = [i for i, (j, _) in enumerate(match) if j < 0]
        extras = [j for j in range(n_got) if j not in used]
        on_edge = lambda st_, pi_: abs(st_ - 0.9071) < 1e-5 or abs(pi_ - 0.7459) < 1e-5
        print(f"filters golden (a): oracle {n_ref} masks, engine {n_got}; oracle masks the engine lacks: {len(missing)}, engine masks the oracle lacks: {len(extras)}")
        assert len(missing) <= 2 and len(extras) <= 4
        for i in missing:
            assert on_edge(float(G["stability_score"][i]), float(G["predicted_iou"][i])), i
        for j in extras:
            assert on_edge(meta[j].stability_score, meta[j].predicted_iou), (j, meta[j].stability_score, meta[j].predicted_iou)
        # the common masks in the same ORDER (a crop's survivors leave the NMS sorted by predicted IoU: two candidates whose scores agree to
        # 1e-5 may swap between two fp32 evaluations)
        pairs = [(i, j) for i, (j, _) in enumerate(match) if j >= 0]
        swaps = 0
        for (ia, ja), (ib, jb) in zip(pairs, pairs[1:]):
            if jb < ja:
                swaps += 1
                assert abs(float(G["predicted_iou"][ia]) - float(G["predicted_iou"][ib])) < 1e-5, (ia, ib)
        print(f"   order: {swaps} adjacent swaps between candidates of equal score")
        assert swaps <= 4
        dev = np.array([1.0 - b for j, b in match if j >= 0])
        st = np.array([meta[j].stability_score for j, _ in match if j >= 0])
        st_ref = np.array([G["stability_score"][i] for i, (j, _) in enumerate(match) if j >= 0])
        print(f"   per-mask |IoU - 1| median {np.median(dev):.2e} max {dev.max():.2e}; stability score abs diff max {np.abs(st - st_ref).max():.2e}")
        assert np.median(dev) <= TOL and dev.max() < 1e-2 and np.abs(st - st_ref).max() < TOL
        # (b) cfgAMG's own filters
        G, meta, got, ref = _amg_vs_golden(eng, "amg_default_grid_cfgamg_seed0.npz",
                                           dict(npoints=32, crop_n_layers=2, pred_iou_thresh=0.0, stability_score_thresh=0.92, box_nms_thresh=0.7, crop_nms_thresh=0.7))
        n_ref = int(G["count"])
        print(f"filters golden (b): oracle {n_ref} masks, engine {len(meta)}")
        assert len(meta) == n_ref
        for i in range(n_ref):
            assert np.allclose([meta[i].point_xy[0], meta[i].point_xy[1]], G["point"][i], atol=1e-3) and np.allclose(list(meta[i].crop_box_xywh), G["crop_box"][i], atol=1e-3)
            iou = (got[i] & ref[i]).sum() / max(1, (got[i] | ref[i]).sum())
            assert 1.0 - iou <= TOL
    finally:
        eng.close()


def test_exact_mode_prompts_of_several_points_and_boxes(engine_exact, image, oracle_feats, oracle_large):
    """saber_decode_prompts (a box = its two corner points with labels 2 / 3, then clicks, then upstream's padding point: 9 / 10 decoder
    tokens) against oracle/sam2_ref.prompt_encoder + mask_decoder on the oracle's own features; the bf16 precision refuses such prompts
    loudly; one point per prompt is saber_decode_points."""
    from oracle import sam2_ref
    eng = engine_exact
    cfg, Wt = oracle_large
    eng.set_precision("exact")
    eng.encode(torch.from_numpy(image).cuda())
    for pts, lab, multimask in (
            ([[[200.0, 240.0], [700.0, 820.0], [450.0, 500.0]], [[100.0, 90.0], [400.0, 380.0], [250.0, 300.0]]], [[2, 3, 1], [2, 3, 0]], False),     # box + click
            ([[[300.0, 300.0], [340.0, 310.0]], [[800.0, 200.0], [760.0, 260.0]], [[512.0, 512.0], [10.0, 1000.0]]], [[1, 1], [1, 0], [1, -1]], False),   # two clicks
            ([[[128.0, 900.0], [600.0, 1010.0]]], [[2, 3]], True)):                                                                        # box alone
        p = torch.tensor(pts, dtype=torch.float32)
        l = torch.tensor(lab, dtype=torch.int64)
        with torch.no_grad():
            sp, de = sam2_ref.prompt_encoder(Wt, p, l, None)
            o_low, o_iou, o_obj, _, _ = sam2_ref.mask_decoder(Wt, oracle_feats, sp, de, multimask)
        low, iou, obj = eng.decode_prompts(p.cuda(), l.to(torch.int32).cuda(), slot=0, multimask=multimask)
        e_low = rel_rms(low.cpu(), o_low)
        e_iou = (iou.cpu() - o_iou).abs().max().item()
        print(f"{p.shape[1]} points per prompt, multimask={multimask}: low-res logits {e_low:.2e}, iou abs {e_iou:.2e}, obj abs {(obj.cpu() - o_obj.reshape(-1)).abs().max().item():.2e}")
        assert e_low < 1e-3 and e_iou < 1e-3
    eng.set_precision("bf16")
    with pytest.raises(RuntimeError, match="exact precision"):
        eng.decode_prompts(torch.zeros(1, 2, 2, device="cuda"), torch.ones(1, 2, dtype=torch.int32, device="cuda"), slot=0)
    p1 = torch.tensor([[[300.0, 400.0]]], device="cuda"); l1 = torch.ones(1, 1, dtype=torch.int32, device="cuda")
    a = eng.decode_prompts(p1, l1, slot=0, multimask=True)[0]
    b = eng.decode_points(p1[:, 0].contiguous(), slot=0, multimask=True)[0]
    assert torch.equal(a, b)
