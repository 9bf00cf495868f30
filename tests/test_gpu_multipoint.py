"""GPU: the 16-token route of the 16-bit decoder (include/saber_amd.h: saber_engine_set_multipoint; csrc/decoder_t16.hip): prompts of
2..9 points - a box, a box plus clicks, several clicks - on the handle's bf16 / fp16 kernels instead of the exact precision mode.

The image -> tokens kernel against fp64 on the same 16-bit operands; whole decodes against the exact mode on the SAME slot (identical
features), and two prompts against the fp32 oracle on the engine's own features; masking and isolation of the padding tokens; the switch
leaves every existing contract alone; the video predictor and the drop-in adapter on it."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.op16 import DTYPE, operand_type

pytestmark = pytest.mark.gpu

# fp16 operands against the exact mode on identical features: the target was tests/test_gpu_fp16.py's TOL = 1e-3 for the decoder alone;
# measured on the box prompts: low-res logits 8.3e-4 (three masks) and 1.27e-3 (single-mask dynamic selection), IoU 1.05e-3 with a mask prompt
TOL_16 = 2e-3
BF16_REL, BF16_AGREE = 1.1e-2, 0.997       # smoke(): bf16 operands against fp32


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def rel_rms(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12)).item()


# ------------------------------------------------------------------------------------------------ kernel: dec_i2t16
def i2t16_inputs(P, shared, nvalid, op, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s, scale=1.0: torch.randn(*s, device="cuda", generator=g) * scale
    T = DTYPE[op]
    return dict(X=r(1 if shared else P, 4096, 256).to(T), Kt=r(P, 128, 256, scale=0.08).to(T), peq=r(4096, 128).to(T), tk=r(P * 16, 128), kscale=0.3,
                cb=r(P, 128), VtT=r(P, 256, 128, scale=0.5).to(T), bo=r(256), gamma=1.0 + 0.1 * r(256), beta=0.1 * r(256), P=P, shared=shared,
                nvalid=nvalid, op=op)


def i2t16_launch(lib, d):
    out = torch.zeros(d["P"], 4096, 256, device="cuda", dtype=DTYPE[d["op"]])
    with operand_type(lib, d["op"]):
        st = lib.saber_k_dec_i2t16(ptr(d["X"]), 0 if d["shared"] else 4096 * 256, ptr(d["peq"]), ptr(d["Kt"]), ptr(d["tk"]), d["kscale"], ptr(d["cb"]),
                                   ptr(d["VtT"]), ptr(d["bo"]), ptr(d["gamma"]), ptr(d["beta"]), 1e-5, ptr(out), d["P"], d["nvalid"], None)
        assert st == 0, lib.saber_k_last_error().decode()
        torch.cuda.synchronize()
    return out


def i2t16_ref(d):
    """LN(x + softmax over the valid tokens of each head(x Kt^T + kscale tk . peq + cb) Vt + bo) in fp64; scores in the exp2 domain; the
    kernel rounds the scaled projection tk and the softmax weights to the operand type for its MFMAs"""
    P, T, nv = d["P"], DTYPE[d["op"]], d["nvalid"]
    X = d["X"].double().expand(P, -1, -1)
    tkb = (d["tk"] * d["kscale"]).to(T).double().view(P, 16, 8, 16)                       # [p][t][h][i]
    pe = torch.einsum("pthi,nhi->pnht", tkb, d["peq"].double().view(4096, 8, 16))         # [p][n][h][t]
    S = (X @ d["Kt"].double().transpose(1, 2)).view(P, 4096, 8, 16) + pe + d["cb"].double().view(P, 1, 8, 16)
    S[..., nv:] = -float("inf")
    Pm = torch.softmax(S * np.log(2.0), dim=-1).reshape(P, 4096, 128)
    Y = Pm.to(T).double() @ d["VtT"].double().transpose(1, 2)
    return F.layer_norm(X + Y + d["bo"].double(), (256,), d["gamma"].double(), d["beta"].double(), 1e-5)


@pytest.mark.parametrize("op", ["bf16", "fp16"])
@pytest.mark.parametrize("shared,nvalid", [(False, 9), (True, 12), (False, 16), (True, 9), (False, 12)])
def test_dec_i2t16_against_fp64_and_blind_to_padding(gpu_lib, op, shared, nvalid):
    P = 3
    d = i2t16_inputs(P, shared, nvalid, op, 40 + nvalid)
    out = i2t16_launch(gpu_lib, d)
    ref = i2t16_ref(d)
    err = (out.double() - ref).abs()
    rms = err.pow(2).mean().sqrt().item()
    print(f"dec_i2t16 {op} shared={shared} nvalid={nvalid}: max abs {err.max().item():.3e}, rms {rms:.3e}")
    bmax, brms = (0.04, 4e-3) if op == "bf16" else (0.01, 1e-3)          # dec_i2t's bounds (tests/test_gpu_kernels.py check_i2t)
    assert err.max().item() < bmax and rms < brms
    if nvalid < 16:
        # the padding columns' operands filled with large finite garbage, twice: not one output bit may move
        outs = []
        for k, big in enumerate((3.0e3, -7.0e3)):
            e = dict(d)
            e["Kt"] = d["Kt"].clone(); e["Kt"].view(P, 8, 16, 256)[:, :, nvalid:] = big
            e["VtT"] = d["VtT"].clone(); e["VtT"].view(P, 256, 8, 16)[..., nvalid:] = big * (1 - 2 * k)
            e["tk"] = d["tk"].clone(); e["tk"].view(P, 16, 128)[:, nvalid:] = big
            e["cb"] = d["cb"].clone(); e["cb"].view(P, 8, 16)[..., nvalid:] = big
            outs.append(i2t16_launch(gpu_lib, e))
        assert torch.equal(outs[0], out) and torch.equal(outs[1], out)


# ------------------------------------------------------------------------------------------------ decoder alone
def _handle(W, operands, max_prompts=32):
    from saber_amd.engine import Engine
    return Engine("large", device=0, weights=W, max_images=1, max_prompts=max_prompts, precision="exact", operands=operands, multipoint=True)


def _cases(rng, n):
    """(name, pts (n,K,2), labels (n,K)): prompt 0 is the named case, the rest random prompts of the same structure"""
    def box(m):
        a = rng.uniform(0, 1024, (m, 2, 2)).astype(np.float32)
        return np.concatenate([a.min(1, keepdims=True), a.max(1, keepdims=True)], 1)
    out = []
    p = box(n); out.append(("box", p, np.tile(np.array([[2, 3]], np.int32), (n, 1))))
    p = np.concatenate([box(n), rng.uniform(0, 1024, (n, 1, 2)).astype(np.float32)], 1)
    out.append(("box+click", p, np.concatenate([np.tile(np.array([[2, 3]], np.int32), (n, 1)), rng.integers(0, 2, (n, 1)).astype(np.int32)], 1)))
    p = rng.uniform(0, 1024, (n, 2, 2)).astype(np.float32)
    out.append(("click + label -1", p, np.stack([np.ones(n, np.int32), np.full(n, -1, np.int32)], 1)))
    p = rng.uniform(0, 1024, (n, 9, 2)).astype(np.float32)
    lab = rng.integers(0, 2, (n, 9)).astype(np.int32); lab[:, :2] = [2, 3]
    out.append(("box + 7 clicks (K = 9)", p, lab))
    return out


def _decode(eng, precision, pts, lab, multimask, mask):
    eng.set_precision(precision)
    low, iou, obj = eng.decode_prompts(torch.from_numpy(pts).cuda(), torch.from_numpy(lab).cuda(), slot=0, multimask=multimask, mask_input=mask)
    torch.cuda.synchronize()
    return low, iou, obj


@pytest.mark.parametrize("operands", ["fp16", "bf16"])
def test_decoder_16_tokens_against_exact_mode(large_weights, image, operands):
    """16-bit decode (max_prompts 32: chunks of 16 prompts, 64 prompts = 4 chunks) against the exact-mode decode of the same slot"""
    cfg, W = large_weights
    eng = _handle(W, operands)
    try:
        eng.set_precision(operands)
        eng.encode(torch.from_numpy(image).cuda())
        rng = np.random.default_rng(17)
        n = 64
        for name, pts, lab in _cases(rng, n):
            first = None
            for use_mask in (False, True):
                mask = None
                if use_mask:       # a clamped logit mask prompt: the first pass's best mask (SAM2ImagePredictor._predict's +-32 clamp)
                    mask = torch.clamp(first[:, 0], -32, 32).contiguous()
                for multimask in (True, False):
                    low, iou, obj = _decode(eng, operands, pts, lab, multimask, mask)
                    r_low, r_iou, r_obj = _decode(eng, "exact", pts, lab, multimask, mask)
                    if first is None and multimask:
                        first = r_low
                    e_low = rel_rms(low, r_low)
                    e_iou = (iou - r_iou).abs().max().item()
                    agree = ((low > 0) == (r_low > 0)).float().mean().item()
                    print(f"{operands} {name} mask={use_mask} multimask={multimask}: low-res rel-rms {e_low:.2e}, iou abs {e_iou:.2e}, "
                          f"pixel agreement {agree:.5f}, obj abs {(obj - r_obj).abs().max().item():.2e}")
                    if operands == "fp16":
                        assert e_low < TOL_16 and e_iou < TOL_16
                    else:
                        assert e_low < BF16_REL and agree > BF16_AGREE
        assert eng.precision == "exact"
    finally:
        eng.close()


def test_decoder_16_tokens_against_oracle_and_isolation(large_weights, oracle_large, image):
    """two prompts (a box + a click, two clicks one of which is not a point) against oracle/sam2_ref on the engine's own features, as smoke()
    does; the padding tokens and a label -1 point's coordinates change no bit; the 8-token route and the switch's contracts are untouched"""
    from oracle import sam2_ref
    from saber_amd.engine import Engine
    cfg, W = large_weights
    _, Wt = oracle_large
    eng = Engine("large", device=0, weights=W, max_images=1, max_prompts=8, precision="fp16", multipoint=True)
    plain = Engine("large", device=0, weights=W, max_images=1, max_prompts=8, precision="fp16")
    try:
        img = torch.from_numpy(image).cuda()
        eng.encode(img)
        plain.encode(img)
        feats = {k: v.cpu()[None] for k, v in eng.get_features(0).items()}
        for pts, lab in (([[[200.0, 240.0], [700.0, 820.0], [450.0, 500.0]]], [[2, 3, 1]]), ([[[300.0, 300.0], [340.0, 310.0]]], [[1, -1]])):
            p, l = torch.tensor(pts), torch.tensor(lab, dtype=torch.int64)
            low, iou, _ = eng.decode_prompts(p.cuda(), l.to(torch.int32).cuda(), slot=0, multimask=True)
            with torch.no_grad():
                sp, de = sam2_ref.prompt_encoder(Wt, p, l, None)
                r_low, r_iou, _, _, _ = sam2_ref.mask_decoder(Wt, feats, sp, de, True)
            err, agree = rel_rms(low.cpu(), r_low), ((low.cpu() > 0) == (r_low > 0)).float().mean().item()
            print(f"K = {p.shape[1]} vs the fp32 oracle: low-res rel-rms {err:.3e}, pixel agreement {agree:.5f}, iou abs {(iou.cpu() - r_iou).abs().max().item():.2e}")
            assert err < 1.5e-3 and agree > 0.9995            # smoke()'s fp16 bounds
        # isolation: a K = 2 decode gives the same bits before and after a K = 9 decode on the same handle
        rng = np.random.default_rng(2)
        p2 = torch.from_numpy(rng.uniform(0, 1024, (5, 2, 2)).astype(np.float32)).cuda()
        l2 = torch.tensor([[1, 0]] * 5, dtype=torch.int32, device="cuda")
        a = eng.decode_prompts(p2, l2, slot=0, multimask=True)
        p9 = torch.from_numpy(rng.uniform(0, 1024, (7, 9, 2)).astype(np.float32)).cuda()
        eng.decode_prompts(p9, torch.ones(7, 9, dtype=torch.int32, device="cuda"), slot=0, multimask=False)
        b = eng.decode_prompts(p2, l2, slot=0, multimask=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        # the coordinates of a label -1 point do not change any bit
        l3 = torch.tensor([[1, -1]] * 5, dtype=torch.int32, device="cuda")
        c = eng.decode_prompts(p2, l3, slot=0, multimask=False)
        q = p2.clone(); q[:, 1] = torch.tensor([3.0, 1000.0], device="cuda")
        d = eng.decode_prompts(q, l3, slot=0, multimask=False)
        assert all(torch.equal(x, y) for x, y in zip(c, d))
        # saber_get_decoder_tokens after a 16-token decode: the first 8 rows of each prompt of the last chunk (max_prompts / 2 = 4 prompts)
        eng.decode_prompts(p2[:4].contiguous(), l3[:4].contiguous(), slot=0, multimask=False)
        toks = torch.zeros(4, 8, 256, device="cuda")
        eng._check(eng.lib.saber_get_decoder_tokens(eng.h, 4, ptr(toks), None))
        torch.cuda.synchronize()
        assert torch.isfinite(toks).all() and toks.abs().sum(-1).min().item() > 0
        with pytest.raises(ValueError):
            eng._check(eng.lib.saber_get_decoder_tokens(eng.h, 5, ptr(torch.zeros(5, 8, 256, device="cuda")), None))
        eng.check_finite()
        # one point per prompt stays on the 8-token route, bit for bit, and decode_points is that of a handle without the switch
        p1 = torch.tensor([[[300.0, 400.0]], [[700.0, 120.0]]], device="cuda"); l1 = torch.ones(2, 1, dtype=torch.int32, device="cuda")
        x = eng.decode_prompts(p1, l1, slot=0, multimask=True)
        y = eng.decode_points(p1[:, 0].contiguous(), slot=0, multimask=True)
        z = plain.decode_points(p1[:, 0].contiguous(), slot=0, multimask=True)
        assert all(torch.equal(u, v) for u, v in zip(x, y)) and all(torch.equal(u, v) for u, v in zip(y, z))
        # switch off: the documented refusal; K = 10 and max_prompts = 1 are invalid
        with pytest.raises(RuntimeError, match="exact precision"):
            plain.decode_prompts(p2, l2, slot=0)
        eng.set_multipoint(False)
        assert not eng.multipoint
        with pytest.raises(RuntimeError, match="exact precision"):
            eng.decode_prompts(p2, l2, slot=0)
        eng.set_multipoint(True)
        with pytest.raises(ValueError):
            eng.decode_prompts(torch.zeros(1, 10, 2, device="cuda"), torch.ones(1, 10, dtype=torch.int32, device="cuda"), slot=0)
    finally:
        eng.close()
        plain.close()
    one = Engine("tiny", device=0, max_images=1, max_prompts=1, precision="fp16")
    try:
        with pytest.raises(ValueError):
            one.set_multipoint(True)
    finally:
        one.close()


# ------------------------------------------------------------------------------------------------ video predictor and adapter
def test_video_box_and_clicks_on_16_bit_kernels():
    """VideoPredictor on a tiny fp16 handle with multipoint on and no exact weight copies: a box, a box + a click, clicks over two calls,
    against oracle/sam2_video_ref with the bounds of tests/test_gpu_video.py::test_box_and_several_clicks_against_oracle"""
    from oracle import sam2_video_ref as V
    from saber_amd.adapters.sam2.video import VideoPredictor, load_tomogram_frames
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import param_specs, seeded_weights
    cfg = get_config("tiny")
    W = seeded_weights(cfg, 0, video=True)
    W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] = W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] + np.float32(3.0)
    img_keys = set(param_specs(cfg).keys())
    eng = Engine("tiny", device=0, weights={k: v for k, v in W.items() if k in img_keys}, max_images=3, max_prompts=8, precision="fp16", multipoint=True)
    assert not eng.has_exact
    try:
        vp = VideoPredictor(eng, W, num_maskmem=2)
        tomo = np.random.default_rng(5).uniform(-1, 1, (5, 128, 128)).astype(np.float32)
        P = V.VideoPredictorRef(W, cfg, num_maskmem=2)
        for case in ("box", "box+click", "two calls"):
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
            assert eng.precision == "fp16"
            e0 = rel_rms(vp.temp[7][1]["pred_masks"].cpu(), P.temp[7][1]["pred_masks"][0, 0])
            ep = rel_rms(vp.temp[7][1]["obj_ptr"].cpu(), P.temp[7][1]["obj_ptr"])
            print(f"{case}: prompted frame low-res rel-rms {e0:.3e}, pointer {ep:.3e}")
            assert e0 < 2.2e-2 and ep < 1.4e-2
            ref = {t: lg for t, _, lg in P.propagate_in_video(1, max_frame_num_to_track=1)}
            got = {t: lg for t, _, lg in vp.propagate_in_video(1, max_frame_num_to_track=1)}
            assert sorted(ref) == sorted(got) == [1, 2]
            for t in ref:
                g, r = got[t][0, 0].cpu() > 0, ref[t][0, 0] > 0
                iou = float((g & r).sum()) / max(1.0, float((g | r).sum()))
                print(f"{case}: frame {t} mask IoU {iou:.4f}")
                assert iou > 0.97 or (not g.any() and not r.any())
        assert eng.precision == "fp16"
    finally:
        eng.close()


def test_adapter_box_prompt_in_default_configuration():
    import os
    os.environ["SABER_AMD_SEEDED_WEIGHTS"] = "1"
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.amg import cfgAMG
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    ad = SAM2Adapter(SAM2AdapterConfig(cfg="tiny", amg_cfg=cfgAMG(sam2_cfg="tiny")), device="cuda")
    rng = np.random.default_rng(3)
    vol = np.clip(rng.normal(32768, 3000, (3, 256, 256)), 0, 65535).astype(np.float32)
    ad.set_volume(vol)
    f, ids, logits = ad.add_new_points_or_box(1, 1, box=[200.0, 220.0, 700.0, 640.0])
    assert f == 1 and list(ids) == [1] and tuple(logits.shape) == (1, 1, 1024, 1024)
    assert torch.isfinite(torch.as_tensor(logits)).all()
    assert ad._video().eng.multipoint and ad._video().eng.precision in ("bf16", "fp16")
