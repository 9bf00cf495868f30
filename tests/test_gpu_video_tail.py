"""GPU: the object-batched tail of a tracked video frame (VideoPredictor(batch_objects=True), batch_tail on): SAM heads enqueued for all
objects, one host wait, object pointers / memory encoder / hole fill / resize once per frame.  The per-object route stays, so the yardstick
of every test here is EXACT equality with it (torch.equal on the raw 16-bit / fp32 storage): the two batched convolution entries against
that many calls of the single entries, the batched GEMM at the shapes the tail gives it, then propagate_in_video with the tail on against
the same handle's per-object route."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.op16 import DTYPE, OPS, operand_type

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
OBJ_BLOCK = 4                      # objects per thread of the batched convolution kernels (csrc/video_ops.hip)
BATCHES = (1, OBJ_BLOCK - 1, OBJ_BLOCK + 1, 17)          # below, across and well above the object block
CANARY = 0x7FC00123                # a NaN no kernel produces


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ck(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _canary(n):
    return torch.full((n,), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)


def _check_planes(out, ref, B, stride, plane):
    """out: the flat batched output (B blocks of `stride` floats over a canary), ref: (B, plane) from the single entry"""
    torch.cuda.synchronize()
    blocks = out[:B * stride].view(B, stride)
    assert not torch.isnan(blocks[:, :plane]).any(), "a plane element was not written"
    assert torch.equal(blocks[:, :plane], ref)
    gaps = torch.cat([blocks[:, plane:].reshape(-1), out[B * stride:]])
    assert gaps.numel() >= (8 if stride > plane else 0) and bool((gaps.view(torch.int32) == CANARY).all()), "a gap element was overwritten"
    if B > 1:
        assert not torch.equal(blocks[0, :plane], blocks[1, :plane])


# ------------------------------------------------------------------------------------------------ the two convolutions over a batch
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("H,W,Cin,Cout", [(8, 8, 1, 4), (6, 10, 4, 16), (8, 8, 16, 64), (8, 8, 64, 256)])
def test_conv3x3s2_t_batched_is_the_single_call_per_object(gpu_lib, H, W, Cin, Cout, pad):
    """outputs of 4 x 4 / 3 x 5 pixels: every pixel of the first row and column has skipped taps"""
    lib = gpu_lib
    g = _gen(H * W + Cin + Cout)
    wt = torch.randn((3, 3, Cin, Cout), generator=g, device="cuda") * (9 * Cin) ** -0.5
    b = torch.randn(Cout, generator=g, device="cuda")
    in_plane, out_plane = H * W * Cin, (H // 2) * (W // 2) * Cout
    si, so = in_plane + pad, out_plane + pad
    for B in BATCHES:
        x = torch.randn((B, si), generator=g, device="cuda")
        out = _canary(B * so + 8)
        ref = torch.zeros((B, out_plane), device="cuda")
        ck(lib, lib.saber_k_conv3x3s2_t_batched(ptr(x), si, H, W, Cin, ptr(wt), ptr(b), Cout, ptr(out), so, B, None))
        for i in range(B):
            ck(lib, lib.saber_k_conv3x3s2_t(ptr(x[i]), H, W, Cin, ptr(wt), ptr(b), Cout, ptr(ref[i]), None))
        _check_planes(out, ref, B, so, out_plane)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("H,W,Cc", [(9, 12, 8), (64, 64, 256)])
def test_dwconv7_t_batched_is_the_single_call_per_object(gpu_lib, H, W, Cc, pad):
    lib = gpu_lib
    g = _gen(H * W + Cc)
    wt = torch.randn((49, Cc), generator=g, device="cuda") / 7
    b = torch.randn(Cc, generator=g, device="cuda")
    plane = H * W * Cc
    st = plane + pad
    for B in BATCHES:
        x = torch.randn((B, st), generator=g, device="cuda")
        out = _canary(B * st + 8)
        ref = torch.zeros((B, plane), device="cuda")
        ck(lib, lib.saber_k_dwconv7_t_batched(ptr(x), st, H, W, Cc, ptr(wt), ptr(b), ptr(out), st, B, None))
        for i in range(B):
            ck(lib, lib.saber_k_dwconv7_t(ptr(x[i]), H, W, Cc, ptr(wt), ptr(b), ptr(ref[i]), None))
        _check_planes(out, ref, B, st, plane)


def test_batched_convolutions_refuse_bad_arguments(gpu_lib):
    lib = gpu_lib
    x = torch.zeros(4 * 8 * 8 * 8, device="cuda")
    w = torch.zeros(49 * 8 * 8, device="cuda")
    b = torch.zeros(8, device="cuda")
    o = torch.zeros(4 * 8 * 8 * 8, device="cuda")

    def conv(inp=x, si=256, H=8, W=8, Cin=4, wt=w, bias=b, Cout=8, out=o, so=128, batch=2):
        return lib.saber_k_conv3x3s2_t_batched(ptr(inp), si, H, W, Cin, ptr(wt), ptr(bias), Cout, ptr(out), so, batch, None)

    def dw(inp=x, si=512, H=8, W=8, Cc=8, wt=w, bias=b, out=o, so=512, batch=2):
        return lib.saber_k_dwconv7_t_batched(ptr(inp), si, H, W, Cc, ptr(wt), ptr(bias), ptr(out), so, batch, None)

    ck(lib, conv())
    ck(lib, dw())
    ck(lib, conv(si=4, so=4, batch=1))           # one object: the strides are not used for a second plane
    for fn, bad in ((conv, [dict(batch=0), dict(batch=-1), dict(si=252), dict(so=124), dict(si=258), dict(so=130), dict(H=7), dict(W=7), dict(Cout=6),
                                dict(inp=None), dict(wt=None), dict(bias=None), dict(out=None)]),
                    (dw, [dict(batch=0), dict(si=508), dict(so=508), dict(si=514), dict(so=514), dict(Cc=6), dict(inp=None), dict(wt=None), dict(bias=None),
                          dict(out=None)])):
        for kw in bad:
            assert fn(**kw) != 0, (fn.__name__, kw)
            assert len(lib.saber_k_last_error()) > 0, (fn.__name__, kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the batched GEMM at the tail's shapes
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("M,K,N,act,f32_out,bias,shared_a,res", [
    (4096, 256, 1024, ACT_GELU, False, True, False, False),          # fuser pwconv1
    (4096, 1024, 256, ACT_NONE, True, True, False, False),           # fuser pwconv2
    (4096, 256, 64, ACT_NONE, False, True, False, False),            # out_proj
    (4096, 256, 256, ACT_NONE, True, True, True, True),              # pix_feat_proj: the frame's features shared, a residual per object
    (1, 256, 256, ACT_RELU, False, True, False, False),              # obj_ptr_proj: one row per object
])
def test_gemm_ld_batched_at_the_tail_shapes(gpu_lib, op, M, K, N, act, f32_out, bias, shared_a, res):
    lib, B = gpu_lib, 3
    g = _gen(M + K + N)
    A = (torch.randn((1 if shared_a else B, M, K), generator=g, device="cuda")).to(DTYPE[op]).view(torch.int16)
    W = (torch.randn((N, K), generator=g, device="cuda") * K ** -0.5).to(DTYPE[op]).view(torch.int16)
    bv = torch.randn(N, generator=g, device="cuda")
    r = torch.randn((B, M, N), generator=g, device="cuda") if res else None
    dt = torch.float32 if f32_out else torch.int16
    out = torch.zeros((B, M, N), dtype=dt, device="cuda")
    ref = torch.ones((B, M, N), dtype=dt, device="cuda")
    with operand_type(lib, op):
        ck(lib, lib.saber_k_gemm_ld_batched(ptr(A), K, 0 if shared_a else M * K, ptr(W), K, 1, ptr(bv) if bias else None, ptr(r), M * N if res else 0,
                                            ptr(out) if f32_out else None, M * N if f32_out else 0, None if f32_out else ptr(out), 0 if f32_out else M * N,
                                            M, N, K, act, B, None))
        for i in range(B):
            ck(lib, lib.saber_k_gemm_ld(ptr(A[0 if shared_a else i]), K, ptr(W), K, 1, ptr(bv) if bias else None, ptr(r[i]) if res else None,
                                        ptr(ref[i]) if f32_out else None, None if f32_out else ptr(ref[i]), M, N, K, act, None))
    torch.cuda.synchronize()
    assert torch.equal(out, ref), (op, M, K, N)
    assert not torch.equal(out[0], out[1])


# ------------------------------------------------------------------------------------------------ end to end
ABSENT_BIAS = 1.39                 # object-score bias offset at which the seeded head predicts one object present and two absent: test_an_absent_object_bit_identical


def _disc(cy, cx, r):
    yy, xx = np.mgrid[:128, :128]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 < r ** 2).astype(np.float32)


@pytest.fixture(scope="module")
def tail_case():
    """the tiny trunk with seeded video weights and an object-score bias offset (+3: the seeded head otherwise predicts 'absent' everywhere),
    num_maskmem = 2, a (7, 128, 128) tomogram, windows of 3 frames; per (operand type, offset) one engine with three predictors on it:
    per object / batched attention with the per-object tail / batched attention and tail"""
    from saber_amd.adapters.sam2.video import VideoPredictor, load_tomogram_frames
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import param_specs, seeded_weights
    cfg = get_config("tiny")
    tomo = np.random.default_rng(42).uniform(-1, 1, (7, 128, 128)).astype(np.float32)
    seeds = [_disc(64, 64, 128 // 6), _disc(40, 90, 14), _disc(95, 40, 12)]
    engines, made = {}, {}

    def get(op, offset=3.0):
        if (op, offset) not in made:
            W = seeded_weights(cfg, 0, video=True)
            k = "sam_mask_decoder.pred_obj_score_head.layers.2.bias"
            W[k] = W[k] + np.float32(offset)
            img = {n: v for n, v in W.items() if n in set(param_specs(cfg).keys())}
            eng = engines[(op, offset)] = Engine("tiny", device=0, weights=img, max_images=3, max_prompts=8, **({"precision": "fp16"} if op == "fp16" else {}))
            off = VideoPredictor(eng, W, num_maskmem=2, batch_objects=False)
            attn = VideoPredictor(eng, W, num_maskmem=2, batch_objects=True, batch_tail=False)
            on = VideoPredictor(eng, W, num_maskmem=2, batch_objects=True)
            assert on.batch_objects and on.batch_tail and attn.batch_objects and not attn.batch_tail and not off.batch_objects
            made[(op, offset)] = (off, attn, on)
        return made[(op, offset)]

    yield {"get": get, "engines": engines, "frames": load_tomogram_frames(tomo), "seeds": seeds, "runs": {}}
    for e in engines.values():
        e.close()


def _run(vp, frames, seeds, seed_frames, start=2):
    """add the seeds, propagate forwards then backwards from `start`; everything the run yields and stores, as clones"""
    vp.init_state(frames, video_hw=(128, 128))
    for i, (m, f) in enumerate(zip(seeds, seed_frames), start=1):
        vp.add_new_mask(f, i, m)
    yielded = []
    for reverse in (False, True):
        for t, ids, logits in vp.propagate_in_video(start, None, reverse):
            yielded.append((t, tuple(ids), reverse, logits.clone()))
    stored = {}
    for oid in vp.obj_ids:
        for kind in ("cond", "non_cond"):
            for t, o in vp.out[oid][kind].items():
                stored[(oid, kind, t)] = (o["pred_masks"].clone(), o["obj_ptr"].clone(), float(o["obj"]), _bits(o["mem"]).clone())
    torch.cuda.synchronize()
    return yielded, stored


def _same(a, b):
    ya, sa = a
    yb, sb = b
    assert len(ya) == len(yb) and len(ya) > 0
    for (t, ids, rev, la), (t2, ids2, rev2, lb) in zip(ya, yb):
        assert (t, ids, rev) == (t2, ids2, rev2)
        assert la.shape == lb.shape and torch.equal(la, lb), ("yielded logits", t, rev)
    assert set(sa) == set(sb) and any(k[1] == "non_cond" for k in sa)
    for key in sa:
        for x, y, what in zip(sa[key], sb[key], ("pred_masks", "obj_ptr", "obj", "mem")):
            assert (x == y) if what == "obj" else (x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)), (key, what)


def _reference(case, op, seed_frames, offset=3.0, fill=0, seed_order=(0, 1, 2)):
    """the per-object route's run, once per operand type, seeding plan, offset, hole-fill setting and order of the seeds"""
    key = (op, seed_frames, offset, fill, seed_order)
    if key not in case["runs"]:
        off = case["get"](op, offset)[0]
        off.fill_hole_area = fill
        try:
            case["runs"][key] = _run(off, case["frames"], [case["seeds"][i] for i in seed_order], seed_frames)
        finally:
            off.fill_hole_area = 0
    return case["runs"][key]


@pytest.mark.parametrize("op", OPS)
def test_three_objects_both_directions_bit_identical(tail_case, op):
    ref = _reference(tail_case, op, (2, 2, 2))
    on = tail_case["get"](op)[2]
    _same(_run(on, tail_case["frames"], tail_case["seeds"], (2, 2, 2)), ref)
    stored = ref[1]          # the three objects differ (a batch that wrote object 0's result three times would not pass by accident)
    assert not torch.equal(stored[(1, "non_cond", 4)][0], stored[(2, "non_cond", 4)][0])
    assert not torch.equal(stored[(2, "non_cond", 4)][3], stored[(3, "non_cond", 4)][3])
    assert not torch.equal(stored[(1, "non_cond", 4)][1], stored[(2, "non_cond", 4)][1])


def test_chunks_of_object_batch_bit_identical(tail_case):
    ref = _reference(tail_case, "bf16", (2, 2, 2))
    on = tail_case["get"]("bf16")[2]
    on.object_batch = 2                     # a chunk of 2 and a chunk of 1
    try:
        _same(_run(on, tail_case["frames"], tail_case["seeds"], (2, 2, 2)), ref)
    finally:
        on.object_batch = 16


def test_conditioning_frame_among_tracked_objects_bit_identical(tail_case):
    """object 3 is seeded on frame 4: that frame is a conditioning frame for it and a tracked frame for objects 1 and 2, whose planes are
    stacked with its stored one for the yield"""
    ref = _reference(tail_case, "bf16", (2, 2, 4))
    on = tail_case["get"]("bf16")[2]
    _same(_run(on, tail_case["frames"], tail_case["seeds"], (2, 2, 4)), ref)
    assert (3, "cond", 4) in ref[1] and (1, "non_cond", 4) in ref[1]


def test_hole_filling_bit_identical(tail_case):
    ref = _reference(tail_case, "bf16", (2, 2, 2), fill=8)
    on = tail_case["get"]("bf16")[2]
    on.fill_hole_area = 8
    try:
        _same(_run(on, tail_case["frames"], tail_case["seeds"], (2, 2, 2)), ref)
    finally:
        on.fill_hole_area = 0


def test_switch_off_is_the_per_object_tail_bit_identical(tail_case):
    ref = _reference(tail_case, "bf16", (2, 2, 2))
    _same(_run(tail_case["get"]("bf16")[1], tail_case["frames"], tail_case["seeds"], (2, 2, 2)), ref)


@pytest.mark.parametrize("seed_order", [(0, 1, 2), (2, 1, 0)])
def test_an_absent_object_bit_identical(tail_case, seed_order):
    """With the +3 offset every object is present on every tracked frame (measured object scores of the per-object run, bf16, seeds on frame 2:
    1.56 .. 1.74 over the 18 object-frames), and the branch of an absent object (NO_OBJ_SCORE plane, no_obj_ptr, no_obj_spatial_bias, the second
    out_proj group) would not run.  At ABSENT_BIAS = 1.39 the same run stores, per seed: the large disc 0.006, 0.11, 0.12, 0.12 on frames 3-6
    (present) and -0.006, -0.07 on frames 1, 0; the two small discs -0.04 .. -0.11 everywhere (absent) - so frames 3-6 hold both kinds in one
    chunk.  seed_order (2, 1, 0) makes the present object the chunk's last: the chunk's stacks are then reordered (present objects first).
    The condition is asserted on the reference run, not assumed."""
    ref = _reference(tail_case, "bf16", (2, 2, 2), offset=ABSENT_BIAS, seed_order=seed_order)
    tracked = {key: v[2] for key, v in ref[1].items() if key[1] == "non_cond"}
    print("object scores on tracked frames:", {k: round(v, 3) for k, v in tracked.items()})
    mixed = [t for t in range(7) if {tracked.get((o, "non_cond", t), 0.0) > 0 for o in (1, 2, 3)} == {True, False} and (1, "non_cond", t) in tracked]
    assert mixed, "the case must hold a frame with a present and an absent object"
    big = seed_order.index(0) + 1
    assert all(tracked[(big, "non_cond", t)] > 0 for t in mixed)
    on = tail_case["get"]("bf16", ABSENT_BIAS)[2]
    _same(_run(on, tail_case["frames"], [tail_case["seeds"][i] for i in seed_order], (2, 2, 2)), ref)


def test_one_host_wait_per_tracked_frame(tail_case):
    off, attn, on = tail_case["get"]("bf16")
    eng = tail_case["engines"][("bf16", 3.0)]
    real = eng.check_finite
    for vp, per_frame in ((on, 1), (attn, 3)):
        vp.init_state(tail_case["frames"], video_hw=(128, 128))
        for i, m in enumerate(tail_case["seeds"], start=1):
            vp.add_new_mask(2, i, m)
        calls = []

        def counting():
            calls.append(1)
            return real()

        eng.check_finite = counting
        try:
            tracked_frames = 0
            for reverse in (False, True):
                for t, ids, _ in vp.propagate_in_video(2, None, reverse):
                    tracked_frames += any(t not in vp.out[o]["cond"] for o in ids)
        finally:
            del eng.check_finite
        assert tracked_frames == 6
        assert len(calls) == per_frame * tracked_frames, (per_frame, len(calls), tracked_frames)
