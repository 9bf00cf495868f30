"""GPU: the object-batched memory attention of the video path (VideoPredictor(batch_objects=True)).  The per-object route stays, so the
yardstick of every test here is EXACT equality with it (torch.equal on the raw 16-bit / fp32 storage): the batched kernel entries against
that many calls of the single-problem entries, saber_k_membank_assemble against its torch restatement, then propagate_in_video and
SAM2Adapter.segment_volume with the switch on against the same handle with it off."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.op16 import DTYPE, OPS, operand_type

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_RELU = 0, 2
MB_CHUNK = 16                      # objects per launch of membank_assemble_kernel (csrc/video_ops.hip)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ck(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()


def _rand16(shape, op, gen, scale=1.0):
    """random values of the operand type as the 16-bit patterns the C-ABI takes (held as int16: torch compares and concatenates those)"""
    return (torch.randn(shape, generator=gen, device="cuda") * scale).to(DTYPE[op]).view(torch.int16)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _split(n_q, n_keys):
    qblocks, nkb, split = n_q // 64, (n_keys + 63) // 64, 1
    while qblocks * split < 256 and split * 2 <= nkb and split < 8:
        split *= 2
    return split


# ------------------------------------------------------------------------------------------------ flash256 over a batch
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n_q,n_keys,batches,split", [(128, 100, (1, 3, 5), 2), (64, 31, (1, 3, 5), 1), (4096, 8212, (2,), 4)])
def test_flash256_batched_is_the_single_call_per_object(gpu_lib, op, n_q, n_keys, batches, split):
    lib = gpu_lib
    assert _split(n_q, n_keys) == split
    g = _gen(n_q + n_keys)
    bias = torch.randn(256, generator=g, device="cuda")
    scale = 1.0 / 16.0
    for B in batches:
        Q = _rand16((B, n_q, 256), op, g)
        K = _rand16((B, n_keys, 256), op, g)
        V = _rand16((B, n_keys, 256), op, g)
        need = B * (n_q // 64) * split * 64 * 258
        ws = torch.empty(need, device="cuda")
        ws1 = torch.empty((n_q // 64) * split * 64 * 258, device="cuda")
        for shared_q in (False, True):
            for use_ws in (True, False):
                out = torch.full((B, n_q, 256), 0x7FC1, dtype=torch.int16, device="cuda")            # canaries: every row must be written
                ref = torch.full((B, n_q, 256), 0x7FC2, dtype=torch.int16, device="cuda")
                with operand_type(lib, op):
                    ck(lib, lib.saber_k_flash256_batched(ptr(Q), 0 if shared_q else n_q * 256, ptr(K), n_keys * 256, ptr(V), n_keys * 256, n_q, n_keys, B, scale,
                                                         ptr(bias), ptr(out), n_q * 256, ptr(ws) if use_ws else None, need if use_ws else 0, None))
                    for b in range(B):
                        ck(lib, lib.saber_k_flash256(ptr(Q[0 if shared_q else b]), ptr(K[b]), ptr(V[b]), n_q, n_keys, scale, ptr(bias), ptr(ref[b]),
                                                     ptr(ws1) if use_ws else None, ws1.numel() if use_ws else 0, None))
                torch.cuda.synchronize()
                assert torch.equal(out, ref), (op, n_q, n_keys, B, shared_q, use_ws)
                if B > 1 and not shared_q:
                    assert not torch.equal(out[0], out[1])
        if split > 1:          # a workspace one float too small is an error, not a silent change of the split
            with operand_type(lib, op):
                st = lib.saber_k_flash256_batched(ptr(Q), n_q * 256, ptr(K), n_keys * 256, ptr(V), n_keys * 256, n_q, n_keys, B, scale, ptr(bias), ptr(out),
                                                  n_q * 256, ptr(ws), need - 1, None)
            assert st != 0 and b"workspace" in lib.saber_k_last_error()


# ------------------------------------------------------------------------------------------------ rope with a period
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("rows_per,n_rot", [(4096 + 64, 4096), (4096, 4096)])
def test_rope_batched_is_the_single_call_per_object(gpu_lib, op, rows_per, n_rot):
    lib, B = gpu_lib, 3
    x = torch.randn((B, rows_per, 256), generator=_gen(rows_per), device="cuda")
    for f32_out in (False, True):
        dt = torch.float32 if f32_out else torch.int16
        out = torch.zeros((B, rows_per, 256), dtype=dt, device="cuda")
        ref = torch.ones((B, rows_per, 256), dtype=dt, device="cuda")
        with operand_type(lib, op):
            ck(lib, lib.saber_k_rope_batched(ptr(x), rows_per, B, n_rot, 256, 64, 10000.0, ptr(out) if f32_out else None, None if f32_out else ptr(out), None))
            for b in range(B):
                ck(lib, lib.saber_k_rope(ptr(x[b]), rows_per, n_rot, 256, 64, 10000.0, ptr(ref[b]) if f32_out else None, None if f32_out else ptr(ref[b]), None))
        torch.cuda.synchronize()
        assert torch.equal(out, ref), (op, rows_per, n_rot, f32_out)
        if f32_out and rows_per > n_rot:          # the rows beyond n_rot of EVERY block are copies
            assert torch.equal(out[:, n_rot:], x[:, n_rot:]) and not torch.equal(out[:, :n_rot], x[:, :n_rot])


# ------------------------------------------------------------------------------------------------ memory-bank assembly
def _membank(lib, op, n_mem, n_ptr, B, mem_of=None, shared_ptr_pos=True, seed=0):
    """one saber_k_membank_assemble call against its torch restatement: concatenate, then (mem.view(T).float() + pos).to(T)"""
    T, g = DTYPE[op], _gen(1000 * n_mem + 10 * n_ptr + B + seed)
    n_tables = 7
    pool = [_rand16((4096, 64), op, g) for _ in range(5)]
    tables = torch.randn((n_tables, 4096, 64), generator=g, device="cuda")
    mem_of = mem_of or [[(3 * b + j) % len(pool) for j in range(n_mem)] for b in range(B)]
    idx = [[(b + 2 * j) % n_tables for j in range(n_mem)] for b in range(B)]
    rows = 4 * n_ptr
    tok = _rand16((B, rows, 64), op, g) if n_ptr else None
    pos = torch.randn((1 if shared_ptr_pos else B, rows, 64), generator=g, device="cuda") if n_ptr else None
    Nk = 4096 * n_mem + rows
    Nkp = (Nk + 63) // 64 * 64
    mem = torch.full((B, Nkp, 64), 0x7FC1, dtype=torch.int16, device="cuda")
    kin = torch.full((B, Nkp, 64), 0x7FC1, dtype=torch.int16, device="cuda")
    n = max(1, B * n_mem)
    ptrs = (C.c_void_p * n)(*[pool[m].data_ptr() for row in mem_of for m in row])
    pidx = (C.c_int * n)(*[i for row in idx for i in row])
    with operand_type(lib, op):
        ck(lib, lib.saber_k_membank_assemble(ptrs, pidx, n_mem, ptr(tables), n_tables, ptr(tok), rows * 64, ptr(pos), 0 if shared_ptr_pos else rows * 64, rows, B,
                                             ptr(mem), ptr(kin), None))
    torch.cuda.synchronize()
    for b in range(B):
        m = torch.cat([pool[i] for i in mem_of[b]] + ([tok[b]] if n_ptr else []), 0)
        p = torch.cat([tables[i] for i in idx[b]] + ([pos[0 if shared_ptr_pos else b]] if n_ptr else []), 0)
        k = (m.view(T).float() + p).to(T).view(torch.int16)
        assert torch.equal(mem[b, :Nk], m) and torch.equal(kin[b, :Nk], k), (op, n_mem, n_ptr, B, b)
        assert not mem[b, Nk:].any() and not kin[b, Nk:].any(), "pad rows must be zero"
    return Nk, Nkp


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n_mem", [1, 2, 7])
@pytest.mark.parametrize("n_ptr", [0, 1, 5])
def test_membank_assemble_against_torch(gpu_lib, op, n_mem, n_ptr):
    for B in (1, 3, MB_CHUNK + 1):
        Nk, Nkp = _membank(gpu_lib, op, n_mem, n_ptr, B, shared_ptr_pos=(B != 3))
    if n_ptr == 1:
        assert Nk == 4096 * n_mem + 4 and Nkp - Nk == 60


@pytest.mark.parametrize("op", OPS)
def test_membank_assemble_objects_sharing_a_memory(gpu_lib, op):
    _membank(gpu_lib, op, 2, 1, 2, mem_of=[[0, 1], [2, 0]])             # memory 0 is object 0's first and object 1's second
    _membank(gpu_lib, op, 1, 0, 3, mem_of=[[4], [4], [4]])


def test_membank_assemble_refuses_bad_arguments(gpu_lib):
    lib = gpu_lib
    m = torch.zeros((4096, 64), dtype=torch.int16, device="cuda")
    tables = torch.zeros((2, 4096, 64), device="cuda")
    out = torch.zeros((1, 4096, 64), dtype=torch.int16, device="cuda")
    ptrs = (C.c_void_p * 1)(m.data_ptr())
    assert lib.saber_k_membank_assemble(ptrs, (C.c_int * 1)(2), 1, ptr(tables), 2, None, 0, None, 0, 0, 1, ptr(out), ptr(out), None) != 0      # table index out of range
    assert lib.saber_k_membank_assemble(ptrs, (C.c_int * 1)(0), 8, ptr(tables), 2, None, 0, None, 0, 0, 1, ptr(out), ptr(out), None) != 0      # more than 7 memories
    assert lib.saber_k_membank_assemble((C.c_void_p * 1)(None), (C.c_int * 1)(0), 1, ptr(tables), 2, None, 0, None, 0, 0, 1, ptr(out), ptr(out), None) != 0


# ------------------------------------------------------------------------------------------------ batched GEMM with residual and activation
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("M", [4096, 8212])
@pytest.mark.parametrize("K,N", [(256, 256), (64, 256), (256, 2048)])
def test_gemm_ld_batched_is_the_single_call_per_object(gpu_lib, op, M, K, N):
    lib, B = gpu_lib, 3
    g = _gen(M + K + N)
    A = _rand16((B, M, K), op, g)
    W = _rand16((N, K), op, g, scale=K ** -0.5)
    bias = torch.randn(N, generator=g, device="cuda")
    res = torch.randn((B, M, N), generator=g, device="cuda")
    kpad = 1 if K % 64 == 0 else 0
    for use_res, res_stride, act in ((False, 0, ACT_NONE), (True, M * N, ACT_NONE), (True, 0, ACT_NONE), (False, 0, ACT_RELU)):
        for f32_out in (False, True):
            dt = torch.float32 if f32_out else torch.int16
            out = torch.zeros((B, M, N), dtype=dt, device="cuda")
            ref = torch.ones((B, M, N), dtype=dt, device="cuda")
            with operand_type(lib, op):
                ck(lib, lib.saber_k_gemm_ld_batched(ptr(A), K, M * K, ptr(W), K, kpad, ptr(bias), ptr(res) if use_res else None, res_stride,
                                                    ptr(out) if f32_out else None, M * N if f32_out else 0, None if f32_out else ptr(out), 0 if f32_out else M * N,
                                                    M, N, K, act, B, None))
                for b in range(B):
                    r = res[b if res_stride else 0] if use_res else None
                    ck(lib, lib.saber_k_gemm_ld(ptr(A[b]), K, ptr(W), K, kpad, ptr(bias), ptr(r), ptr(ref[b]) if f32_out else None, None if f32_out else ptr(ref[b]),
                                                M, N, K, act, None))
            torch.cuda.synchronize()
            assert torch.equal(out, ref), (op, M, K, N, use_res, res_stride, act, f32_out)
    assert not torch.equal(out[0], out[1])


# ------------------------------------------------------------------------------------------------ end to end
def _disc(cy, cx, r):
    yy, xx = np.mgrid[:128, :128]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 < r ** 2).astype(np.float32)


@pytest.fixture(scope="module")
def batch_case():
    """the tiny trunk with seeded video weights and the +3 object-score bias (the seeded head otherwise predicts 'absent' everywhere),
    num_maskmem = 2, a (7, 128, 128) tomogram, windows of 3 frames; per operand type one engine with two predictors on it: switch off / on"""
    from saber_amd.adapters.sam2.video import VideoPredictor, load_tomogram_frames
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import param_specs, seeded_weights
    cfg = get_config("tiny")
    W = seeded_weights(cfg, 0, video=True)
    W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] = W["sam_mask_decoder.pred_obj_score_head.layers.2.bias"] + np.float32(3.0)
    img = {k: v for k, v in W.items() if k in set(param_specs(cfg).keys())}
    tomo = np.random.default_rng(42).uniform(-1, 1, (7, 128, 128)).astype(np.float32)
    seeds = [_disc(64, 64, 128 // 6), _disc(40, 90, 14), _disc(95, 40, 12)]
    engines, made = {}, {}

    def get(op):
        if op not in made:
            engines[op] = Engine("tiny", device=0, weights=img, max_images=3, max_prompts=8, **({"precision": "fp16"} if op == "fp16" else {}))
            off = VideoPredictor(engines[op], W, num_maskmem=2, batch_objects=False)
            on = VideoPredictor(engines[op], W, num_maskmem=2, batch_objects=True)
            assert on.f16 == (op == "fp16") and on.batch_objects and not off.batch_objects and on.object_batch == 16
            made[op] = (off, on)
        return made[op]

    yield {"get": get, "tomo": tomo, "frames": load_tomogram_frames(tomo), "seeds": seeds, "runs": {}}
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
        assert torch.equal(la, lb), ("yielded logits", t, rev)
    assert set(sa) == set(sb) and any(k[1] == "non_cond" for k in sa)
    for key in sa:
        for x, y, what in zip(sa[key], sb[key], ("pred_masks", "obj_ptr", "obj", "mem")):
            assert (x == y) if what == "obj" else (x.dtype == y.dtype and torch.equal(x, y)), (key, what)


def _reference(case, op, seed_frames):
    """the per-object route's run, once per operand type and seeding plan"""
    key = (op, seed_frames)
    if key not in case["runs"]:
        case["runs"][key] = _run(case["get"](op)[0], case["frames"], case["seeds"], seed_frames)
    return case["runs"][key]


@pytest.mark.parametrize("op", OPS)
def test_three_objects_both_directions_bit_identical(batch_case, op):
    ref = _reference(batch_case, op, (2, 2, 2))
    on = batch_case["get"](op)[1]
    _same(_run(on, batch_case["frames"], batch_case["seeds"], (2, 2, 2)), ref)
    # the three objects differ (a batch that wrote object 0's result three times would not pass by accident)
    stored = ref[1]
    assert not torch.equal(stored[(1, "non_cond", 4)][0], stored[(2, "non_cond", 4)][0])
    assert not torch.equal(stored[(2, "non_cond", 4)][3], stored[(3, "non_cond", 4)][3])


def test_chunks_of_object_batch_bit_identical(batch_case):
    ref = _reference(batch_case, "bf16", (2, 2, 2))
    on = batch_case["get"]("bf16")[1]
    on.object_batch = 2                     # a chunk of 2 and a chunk of 1
    try:
        _same(_run(on, batch_case["frames"], batch_case["seeds"], (2, 2, 2)), ref)
    finally:
        on.object_batch = 16


def test_mixed_signatures_bit_identical(batch_case):
    """object 3 is seeded on frame 4: on most frames its bank has another shape than the banks of objects 1 and 2 (two groups), and on
    frame 4 it is a conditioning frame for object 3 alone"""
    from saber_amd.adapters.sam2.video import bank_signature
    ref = _reference(batch_case, "bf16", (2, 2, 4))
    on = batch_case["get"]("bf16")[1]
    _same(_run(on, batch_case["frames"], batch_case["seeds"], (2, 2, 4)), ref)
    sig = [bank_signature(on.out[o], 6, False, 2, 7) for o in (1, 2, 3)]
    assert sig[0] == sig[1] != sig[2]


@pytest.mark.parametrize("device_volume", [False, True])
def test_adapter_switch_returns_the_same_volume_and_scores(batch_case, device_volume):
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.predictor import SAM2Adapter
    ad = SAM2Adapter(SAM2AdapterConfig(cfg="tiny"), device="cuda:0")
    ad._video_predictor = batch_case["get"]("bf16")[0]                    # the fixture's weights; the keyword switches the route per call
    got = {}
    for flag in (False, True):
        ad.set_volume(batch_case["tomo"])
        vol = ad.segment_volume(2, masks=batch_case["seeds"], min_presence_score=0.0, batch_objects=flag, device_volume=device_volume)
        got[flag] = (vol.cpu().numpy().copy() if device_volume else vol.copy(), ad.frame_scores.copy())
        assert ad._video_predictor.batch_objects is False                 # restored after the call
    assert got[True][0].shape == batch_case["tomo"].shape and set(np.unique(got[False][0])) - {0} != set()
    assert np.array_equal(got[False][0], got[True][0])
    assert got[False][1].shape == (7, 3) and np.array_equal(got[False][1], got[True][1])
