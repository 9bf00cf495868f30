"""GPU parity tests of the individual gfx950 kernels, called through the kernel-level C-ABI
(include/saber_amd_kernels.h).  The reference for each primitive is the plain formula in fp64 (the same formulas oracle/sam2_ref.py is
built from), evaluated on the 16-bit-rounded operands the kernel sees.

Every kernel with 16-bit operands is compiled twice (csrc/Makefile OP_SRCS: namespaces op_bf16 and op_f16, each with its own register
allocation), so these tests run under both operand types (tests/op16.py).  The bf16 case of a test keeps the id it had before.

Tolerances: 16-bit operands with fp32 accumulation reproduce an fp64 evaluation of the SAME rounded operands to ~1e-5 relative
(summation order only: the same bound for both types); kernels that round an intermediate or the output to the 16-bit type (attention P,
16-bit outputs) are allowed a few units of that type's rounding, 2^-8 relative for bf16 and 2^-11 for fp16.  Each fp16 bound set by such
a rounding is at most 1/4 of the bf16 one and smaller than what one bf16 rounding of the reference costs (op16.check_bound).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.op16 import DTYPE, FP16_OVERFLOW, OPS, U, check_bound, from_dev, operand_type, params, rnd, to_dev

pytestmark = pytest.mark.gpu


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def kcall(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()
    torch.cuda.synchronize()


def amax(t):
    return t.abs().max().item()


def bound16(op, b_bf16, scale):
    """fp16 bound of a max-abs error set by a 16-bit rounding: the bf16 bound scaled by U, at most 3 fp16 roundings of the case's scale
    (one bf16 rounding of a reference whose largest entries fill their binade costs at least 4 of them)"""
    return min(b_bf16 * U["fp16"] / U["bf16"], 3 * U["fp16"] * scale)


def sep_maxabs(ref):
    """max |bf16(ref) - ref|: what one bf16 rounding of the result costs in the max-abs measure"""
    return amax(rnd(ref, "bf16").double() - ref)


def sep_rms(ref):
    return (rnd(ref, "bf16").double() - ref).pow(2).mean().sqrt().item()


@pytest.mark.parametrize(*params("M,N,K,act,use_res,pool4", [
    (300, 432, 144, 0, False, 0), (4096, 576, 2304, 0, True, 0), (1000, 2304, 576, 1, False, 0),
    (5, 1, 256, 0, False, 0), (64, 4, 256, 3, False, 0), (512, 288, 144, 0, False, 1), (777, 128, 64, 2, True, 0),
    (131072, 288, 128, 0, False, 1), (65536 + 8, 200, 64, 0, True, 1),   # q-pool shortcut through the direct-to-LDS kernels
]))
def test_gemm(gpu_lib, op, M, N, K, act, use_res, pool4):
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g)
    A, Ad = rnd(x, op), to_dev(x, op)
    x = torch.randn(N, K, generator=g) / K ** 0.5
    W, Wd = rnd(x, op), to_dev(x, op)
    bias = torch.randn(N, generator=g)
    Mo = M // 4 if pool4 else M
    res = torch.randn(Mo, N, generator=g) if use_res else None
    bias_d, res_d = bias.cuda(), (res.cuda() if use_res else None)  # keep device operands alive across the call
    ref = (A.cuda().double() @ W.cuda().double().T + bias_d.double())
    if act == 1:
        ref = F.gelu(ref)
    elif act == 2:
        ref = F.relu(ref)
    elif act == 3:
        ref = torch.sigmoid(ref)
    if pool4:
        ref = ref.view(Mo, 4, N).max(1).values
    if use_res:
        ref = ref + res_d.double()
    out_f = torch.zeros(Mo, N, dtype=torch.float32, device="cuda")
    out_b = torch.zeros(Mo, N, dtype=torch.int16, device="cuda")
    with operand_type(gpu_lib, op):
        kcall(gpu_lib, gpu_lib.saber_k_gemm(ptr(Ad), ptr(Wd), ptr(bias_d), ptr(res_d), ptr(out_f), ptr(out_b),
                                            M, N, K, act, 0, pool4, 0, 0, None))
    scale = amax(ref) + 1e-6
    check_bound(op, "fp32 out", amax(out_f.double() - ref) / scale, 2e-5)
    got = out_b.view(DTYPE[op]).double()
    if op == "bf16" or ref.numel() >= 64:
        check_bound(op, "16-bit out", amax(got - ref) / scale, 5e-3, 5e-3 / 8, sep_maxabs(ref) / scale)
    else:
        # too few outputs for the max-abs measure to tell the types apart: per element, one fp16 rounding (RNE) + the fp32 bound
        tol = U["fp16"] * ref.abs() + 3e-5 * scale
        e, sep = amax((got - ref) / tol), amax((rnd(ref, "bf16").double() - ref) / tol)
        print(f"16-bit out [fp16]: max |err| / (2^-11 |ref| + 3e-5 max|ref|) = {e:.3f} (bound 1), one bf16 rounding of the reference {sep:.2f}")
        assert sep > 1 and e <= 1


# ---- every route of launch_gemm (csrc/gemm.hip), in its dispatch order.  T = ceil(M/128) ceil(N/128), T256 = ceil(M/256) ceil(N/128),
# T2 = ceil(M/256) ceil(N/256); direct = w_kpad or K % 64 == 0; only16 = a 16-bit output alone (no fp32 output, residual, pool4), N % 8 == 0,
# act none or GELU.
def gemm_route(M, N, K, act, res, f32, w_kpad=0):
    cd = lambda a, b: (a + b - 1) // b
    T, T256, T2 = cd(M, 128) * cd(N, 128), cd(M, 256) * cd(N, 128), cd(M, 256) * cd(N, 256)
    direct = w_kpad or K % 64 == 0
    only16 = not f32 and not res and N % 8 == 0 and act in (0, 1)
    if direct and only16 and T2 >= 1024 and (N >= 1024 or (act == 0 and N >= 384)):
        # saber_k_gemm_ld packs W per K-step (Wpk) for w_kpad, a 16-bit output alone, K % 64 == 0 and M N >= 2^26
        return "p256s_wpk" if (w_kpad and K % 64 == 0 and M * N >= 1 << 26) else "p256s"
    if direct and T256 >= 512:
        return "glds2"
    if direct and T256 >= 256:
        return "glds4"
    return "gemm4" if T >= 384 else "gemm2"


# route: M, N, K, act, residual, fp32 output, entry point (ld = saber_k_gemm_ld with w_kpad = 1); M and N ragged in every case
GEMM_ROUTES = {
    "gemm2": (777, 200, 192, 1, True, True, "gemm"),          # T = 14 < 384
    "gemm4": (8192 + 5, 800, 144, 2, True, True, "gemm"),     # K % 64 != 0 (not direct), T = 455 >= 384
    "glds4": (256 * 56 + 9, 600, 128, 1, False, True, "gemm"),          # 256 <= T256 = 285 < 512
    "glds2": (256 * 130 + 9, 440, 192, 0, True, True, "gemm"),          # T256 = 524 >= 512
    "p256s": (256 * 128 + 77, 2280, 576, 1, False, False, "gemm"),      # T2 = 1161 >= 1024, N >= 1024, 16-bit output alone
    "p256s_wpk": (256 * 120 + 33, 2184, 576, 0, False, False, "ld"),    # T2 = 1089, M N = 67 164 552 >= 2^26: W packed per K-step
}


def _gemm_route_run(lib, op, route, a_scale=1.0, w_scale=1.0, w_cols=None, bias_scale=1.0, a_fn=None, w_fn=None):
    """one launch of a GEMM_ROUTES case; returns (fp64 reference, fp32 output or None, 16-bit output as fp64)"""
    M, N, K, act, use_res, f32, entry = GEMM_ROUTES[route]
    assert gemm_route(M, N, K, act, use_res, f32, entry == "ld") == route
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    A = torch.randn(M, K, device="cuda", generator=g) * a_scale if a_fn is None else a_fn(g, M, K)
    W = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5 if w_fn is None else w_fn(g, N, K)
    if w_cols is not None:
        W[w_cols] *= w_scale
    Ah, Wh = A.to(DTYPE[op]), W.to(DTYPE[op])
    bias = torch.randn(N, device="cuda", generator=g) * bias_scale
    res = torch.randn(M, N, device="cuda", generator=g) * 2 if use_res else None
    ref = Ah.double() @ Wh.double().T + bias.double()
    ref = F.gelu(ref) if act == 1 else F.relu(ref) if act == 2 else ref
    if use_res:
        ref = ref + res.double()
    of = torch.zeros(M, N, device="cuda") if f32 else None
    ob = torch.zeros(M, N, device="cuda", dtype=DTYPE[op])
    with operand_type(lib, op):
        if entry == "ld":
            kcall(lib, lib.saber_k_gemm_ld(ptr(Ah), K, ptr(Wh), K, 1, ptr(bias), ptr(res), ptr(of), ptr(ob), M, N, K, act, None))
        else:
            kcall(lib, lib.saber_k_gemm(ptr(Ah), ptr(Wh), ptr(bias), ptr(res), ptr(of), ptr(ob), M, N, K, act, 0, 0, 0, 0, None))
    return ref, (of.double() if f32 else None), ob.double()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("route", list(GEMM_ROUTES))
def test_gemm_routes(gpu_lib, route, op):
    """each launch_gemm route in both operand types, ragged M and N, against fp64 on the GPU"""
    ref, of, ob = _gemm_route_run(gpu_lib, op, route)
    scale = amax(ref)
    if of is not None:
        check_bound(op, f"{route} fp32 out", amax(of - ref) / scale, 2e-5)
    check_bound(op, f"{route} 16-bit out", amax(ob - ref) / scale, 5e-3, 5e-3 / 8, sep_maxabs(ref) / scale)


def _check_fp16_overflow(what, ref, got16, got32=None):
    """fp16 output of a result partly beyond the type's range: +-inf where |y| >= 65520 (the run-time sentinel SABER_ERR_RANGE reads it; no
    saturating conversion), finite RNE elsewhere (per column: one fp16 rounding + the fp32 accumulation bound + the GELU fit), the fp32
    output unaffected"""
    col = ref.abs().amax(0, keepdim=True)
    slack = 2e-5 * col
    fit = 2.6e-5            # the GELU fit's absolute error (common.h gelu_erf)
    over = ref.abs() >= FP16_OVERFLOW + slack
    under = ref.abs() < FP16_OVERFLOW - slack
    assert over.any() and under.any(), "the case must straddle the fp16 range"
    assert not torch.isnan(got16).any(), what
    assert torch.equal(got16[over], torch.sign(ref[over]) * float("inf")), (what, "an overflow that is not inf")
    fin = got16[under]
    assert torch.isfinite(fin).all(), (what, "inf below the overflow threshold")
    r = (fin - ref[under]).abs() / (U["fp16"] * ref[under].abs() + slack.expand_as(ref)[under] + fit)
    e = r.max().item()
    print(f"{what}: {int(over.sum())} of {ref.numel()} entries beyond the fp16 range are inf; the others within {e:.2f} of (fp16 RNE + fp32 bound)")
    assert e <= 1.0, what
    if got32 is not None:
        e32 = ((got32 - ref).abs() / (2e-5 * col + fit)).max().item()
        print(f"{what}: fp32 output within {e32:.2f} of (2e-5 column max + GELU fit)")
        assert e32 <= 1.0, what


@pytest.mark.parametrize("route", list(GEMM_ROUTES))
def test_gemm_fp16_overflow_is_inf(gpu_lib, route):
    """every third output column scaled so that its entries straddle 65 520"""
    N = GEMM_ROUTES[route][1]
    ref, of, ob = _gemm_route_run(gpu_lib, "fp16", route, w_scale=4.0e4, w_cols=torch.arange(0, N, 3, device="cuda"))
    _check_fp16_overflow(f"{route} overflow", ref, ob, of)


@pytest.mark.parametrize("route", list(GEMM_ROUTES))
def test_gemm_fp16_subnormal_operands(gpu_lib, route):
    """A entries in the fp16 subnormal range [2^-24, 2^-14) (then the same for W), the other operand large enough for O(1) results: the
    kernels run with .amdhsa_float_denorm_mode_16_64 3, so the f16 MFMA must not flush them (the fp32 bound of the normal case, 2e-5)"""
    def subnormal(g, rows, K):
        mag = torch.rand(rows, K, device="cuda", generator=g) * (2.0 ** -14 - 2.0 ** -23) + 2.0 ** -24
        return mag * torch.sign(torch.randn(rows, K, device="cuda", generator=g))

    def large(g, rows, K):
        return torch.randn(rows, K, device="cuda", generator=g) * 2.0 ** 14 / K ** 0.5

    for side, kw in (("A", dict(a_fn=subnormal, w_fn=large)), ("W", dict(a_fn=large, w_fn=subnormal))):
        ref, of, ob = _gemm_route_run(gpu_lib, "fp16", route, bias_scale=0.01, **kw)
        scale = amax(ref)
        assert 0.05 < scale < 100, scale
        if of is not None:
            check_bound("fp16", f"{route} subnormal {side}, fp32 out", amax(of - ref) / scale, 2e-5)
        check_bound("fp16", f"{route} subnormal {side}, 16-bit out", amax(ob - ref) / scale, 5e-3, 5e-3 / 8, sep_maxabs(ref) / scale)


@pytest.mark.parametrize(*params("M,N,K,act", [(777, 1000, 192, 0), (4096, 2304, 576, 1), (300, 264, 64, 0), (2560, 1728, 576, 0), (256 * 9 + 5, 512, 1152, 1)]))
def test_gemm_p256(gpu_lib, op, M, N, K, act):
    """persistent 256x256-tile kernel (16-bit output): forced through the debug flag for small shapes, ragged M / N, several tiles per block"""
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g)
    A, Ad = rnd(x, op), to_dev(x, op)
    x = torch.randn(N, K, generator=g) / K ** 0.5
    W, Wd = rnd(x, op), to_dev(x, op)
    bias = torch.randn(N, generator=g)
    bias_d = bias.cuda()
    ref = A.cuda().double() @ W.cuda().double().T + bias_d.double()
    ref = F.gelu(ref) if act == 1 else F.relu(ref) if act == 2 else ref
    out_b = torch.zeros(M, N, dtype=torch.int16, device="cuda")
    gpu_lib.saber_k_set_debug(128)
    try:
        with operand_type(gpu_lib, op):
            kcall(gpu_lib, gpu_lib.saber_k_gemm(ptr(Ad), ptr(Wd), ptr(bias_d), None, None, ptr(out_b), M, N, K, act, 0, 0, 0, 0, None))
    finally:
        gpu_lib.saber_k_set_debug(0)
    scale = amax(ref) + 1e-6
    check_bound(op, "p256s 16-bit out", amax(out_b.view(DTYPE[op]).double() - ref) / scale, 5e-3, 5e-3 / 8, sep_maxabs(ref) / scale)


def _gemm_act_last_and_res_mod(lib, op):
    g = torch.Generator().manual_seed(3)
    M, N, K = 640, 128, 64
    x = torch.randn(M, K, generator=g)
    A, Ad = rnd(x, op), to_dev(x, op)
    x = torch.randn(N, K, generator=g) / 8
    W, Wd = rnd(x, op), to_dev(x, op)
    bias = torch.randn(N, generator=g)
    res = torch.randn(160, N, generator=g)
    ref = F.gelu(A.double() @ W.double().T + bias.double() + res.double().repeat(4, 1))
    out_f = torch.zeros(M, N, dtype=torch.float32, device="cuda")
    bias_d, res_d = bias.cuda(), res.cuda()
    with operand_type(lib, op):
        kcall(lib, lib.saber_k_gemm(ptr(Ad), ptr(Wd), ptr(bias_d), ptr(res_d), ptr(out_f), None, M, N, K, 1, 1, 0, 0, 160, None))
    check_bound(op, "act_last + res_mod fp32 out (abs)", amax(out_f.cpu().double() - ref), 1e-4)


def test_gemm_act_last_and_res_mod(gpu_lib):
    _gemm_act_last_and_res_mod(gpu_lib, "bf16")


def test_gemm_act_last_and_res_mod_fp16(gpu_lib):
    _gemm_act_last_and_res_mod(gpu_lib, "fp16")


@pytest.mark.parametrize(*params("rows,C,act", [(1000, 144, 0), (333, 576, 0), (64, 1152, 0), (4096, 64, 1), (17, 256, 0), (5001, 144, 0), (4099, 192, 1), (70003, 144, 0)]))
def test_layernorm(gpu_lib, op, rows, C, act):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(rows, C, generator=g) * 3 + 1
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x.double(), (C,), gam.double(), bet.double(), 1e-6)
    if act:
        ref = F.gelu(ref)
    of = torch.zeros(rows, C, device="cuda")
    ob = torch.zeros(rows, C, dtype=torch.int16, device="cuda")
    xd, gd, bd = x.cuda(), gam.cuda(), bet.cuda()
    with operand_type(gpu_lib, op):
        kcall(gpu_lib, gpu_lib.saber_k_layernorm(ptr(xd), ptr(gd), ptr(bd), 1e-6, ptr(of), ptr(ob), rows, C, act, None))
    # act=1: the kernels' GELU is the 9-op fit of the exact erf form (common.h gelu_erf, |error| <= 2.6e-5 absolute)
    check_bound(op, "fp32 out (abs)", amax(of.cpu().double() - ref), 5e-5 if act else 2e-5)
    scale = amax(ref)
    check_bound(op, "16-bit out / max|ref|", amax(from_dev(ob, op).double() - ref) / scale, 0.03, bound16(op, 0.03, 1.0), sep_maxabs(ref) / scale)


def test_layernorm_fp16_overflow_is_inf(gpu_lib):
    """LayerNorm gains of 2e4: the normalised rows times the gain straddle 65 520 in the fp16 output; the fp32 output stays exact"""
    rows, C = 3001, 192
    g = torch.Generator().manual_seed(17)
    x = torch.randn(rows, C, generator=g) * 3 + 1
    gam, bet = torch.randn(C, generator=g) * 2.0e4, torch.randn(C, generator=g)
    ref = F.layer_norm(x.double(), (C,), gam.double(), bet.double(), 1e-6)
    of = torch.zeros(rows, C, device="cuda")
    ob = torch.zeros(rows, C, dtype=torch.float16, device="cuda")
    xd, gd, bd = x.cuda(), gam.cuda(), bet.cuda()
    with operand_type(gpu_lib, "fp16"):
        kcall(gpu_lib, gpu_lib.saber_k_layernorm(ptr(xd), ptr(gd), ptr(bd), 1e-6, ptr(of), ptr(ob), rows, C, 0, None))
    _check_fp16_overflow("layernorm overflow", ref, ob.cpu().double(), of.cpu().double())


def ref_hiera_attention(qkv, n_windows, nk, heads, q_pool, hd=72, key_mask=None):
    t = qkv.view(n_windows, nk, 3, heads, hd).double()
    q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    if q_pool:
        q = q.view(n_windows, nk // 4, 4, heads, hd).max(2).values
    q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    sc = q @ k.transpose(-1, -2) * hd ** -0.5
    if key_mask is not None:
        sc = sc.masked_fill(~key_mask[None, None, None, :], float("-inf"))
    a = torch.softmax(sc, -1) @ v
    return a.transpose(1, 2).reshape(-1, heads * hd)


def _check_attention(op, what, got, ref, b_max, b_rms):
    """max-abs and relative-rms error of a 16-bit attention output (bf16 / fp16 P and output rounding)"""
    scale = amax(ref)
    rms = ref.pow(2).mean().sqrt().item()
    check_bound(op, f"{what} max abs", amax(got - ref), b_max, bound16(op, b_max, scale), sep_maxabs(ref))
    check_bound(op, f"{what} rel-rms", (got - ref).pow(2).mean().sqrt().item() / rms, b_rms, b_rms / 8, sep_rms(ref) / rms)


@pytest.mark.parametrize(*params("n_windows,nk,heads,q_pool", [
    (9, 64, 2, 0), (5, 64, 4, 1), (33, 16, 4, 0), (7, 16, 8, 1), (3, 256, 8, 0), (2, 256, 16, 1), (1, 4096, 8, 0), (2, 128, 2, 0),
    (3, 512, 4, 0), (11, 1024, 2, 0), (21, 256, 8, 0), (2, 4096, 3, 0),   # streaming kernel: several tasks per block, chunked queries
]))
def test_hiera_attention(gpu_lib, op, n_windows, nk, heads, q_pool):
    g = torch.Generator().manual_seed(nk + heads)
    x = torch.randn(n_windows * nk, 3 * heads * 72, generator=g) * 1.5
    qkv, qd = rnd(x, op), to_dev(x, op)
    ref = ref_hiera_attention(qkv.cuda(), n_windows, nk, heads, q_pool)
    out = torch.zeros(ref.shape, dtype=torch.int16, device="cuda")
    with operand_type(gpu_lib, op):
        kcall(gpu_lib, gpu_lib.saber_k_hiera_attention(ptr(qd), ptr(out), n_windows, nk, heads, q_pool, None))
    _check_attention(op, "hiera attention", out.view(DTYPE[op]).double(), ref, 0.03, 6e-3)  # |v| ~ 1.5: 16-bit P and output rounding


@pytest.mark.parametrize(*params("n_windows,nk,heads,hd,q_pool,masked", [
    # tiny/small (head_dim 96) and base+ (56): 8x8 / 4x4 windows, the 14x14 and 7x7 padded windows, global blocks whose token
    # matrix carries the window-padding rows (4900 rows, 4096 of them real keys)
    (9, 64, 1, 96, 0, 0), (5, 64, 2, 96, 1, 0), (33, 16, 2, 96, 0, 0), (7, 16, 4, 56, 1, 0), (26, 196, 4, 96, 0, 0), (11, 196, 8, 96, 1, 0),
    (25, 49, 8, 96, 0, 0), (25, 49, 16, 56, 0, 0), (9, 196, 8, 56, 0, 0), (3, 196, 16, 56, 1, 0), (1, 4900, 4, 96, 0, 1), (2, 4900, 8, 56, 0, 1),
    (3, 196, 8, 72, 0, 0), (2, 300, 2, 72, 0, 1),
]))
def test_hiera_attention_all_trunks(gpu_lib, op, n_windows, nk, heads, hd, q_pool, masked):
    g = torch.Generator().manual_seed(nk + heads + hd)
    x = torch.randn(n_windows * nk, 3 * heads * hd, generator=g) * 1.5
    qkv, qd = rnd(x, op), to_dev(x, op)
    km = kd = None
    if masked:
        km = torch.rand(nk, generator=g) > 0.2
        km[:8] = True
        pad = torch.zeros((nk + 127) // 128 * 128, dtype=torch.uint8)
        pad[:nk] = km.to(torch.uint8)
        kd = pad.cuda()
    ref = ref_hiera_attention(qkv.cuda(), n_windows, nk, heads, q_pool, hd, None if km is None else km.cuda())
    out = torch.zeros(ref.shape, dtype=torch.int16, device="cuda")
    with operand_type(gpu_lib, op):
        kcall(gpu_lib, gpu_lib.saber_k_hiera_attention_ex(ptr(qd), ptr(out), n_windows, nk, heads, hd, q_pool, ptr(kd) if masked else None, None))
    _check_attention(op, f"hiera attention hd {hd}", out.view(DTYPE[op]).double(), ref, 0.03, 6e-3)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n_windows,nk,heads,hd,qk_scale", [(9, 64, 2, 72, 40.0), (5, 64, 2, 96, 100.0), (2, 256, 4, 56, 120.0)])
def test_hiera_attention_large_scores(gpu_lib, n_windows, nk, heads, hd, qk_scale, op):
    """q and k scaled so that the scores before the 1/sqrt(d) scale are of order 1e4 .. 1e6 (all operands and outputs within fp16's range):
    an intermediate kept in the 16-bit type would overflow in fp16 where bf16's range hides it"""
    g = torch.Generator().manual_seed(nk + heads + hd + 1)
    x = torch.randn(n_windows * nk, 3, heads * hd, generator=g) * 0.5
    x[:, :2] *= 3.0 * qk_scale          # (v ~ N(0, 1/4): one-hot weights return single values of v in full, all below 4 as in the normal cases)
    x = x.view(n_windows * nk, 3 * heads * hd)
    qkv, qd = rnd(x, op), to_dev(x, op)
    ref = ref_hiera_attention(qkv.cuda(), n_windows, nk, heads, 0, hd)
    t = qkv.view(n_windows, nk, 3, heads, hd).double()
    pre = torch.einsum("wqhd,wkhd->whqk", t[:, :, 0], t[:, :, 1]).abs().max().item()
    print(f"largest |q . k| before the scale: {pre:.3e}")
    assert pre > 1e4
    out = torch.zeros(ref.shape, dtype=torch.int16, device="cuda")
    with operand_type(gpu_lib, op):
        kcall(gpu_lib, gpu_lib.saber_k_hiera_attention_ex(ptr(qd), ptr(out), n_windows, nk, heads, hd, 0, None, None))
    got = out.view(DTYPE[op]).double()
    assert torch.isfinite(got).all()
    # fp32 scores carry an absolute error ~2^-24 sum |q_i k_i| that grows with the scores: where the two largest scaled scores of a query lie
    # within a few units the softmax weights move with it (accumulation order, not the type), so those queries are left out
    sc = torch.einsum("wqhd,wkhd->whqk", t[:, :, 0], t[:, :, 1]) * hd ** -0.5
    top = sc.topk(2, dim=-1).values
    keep = (top[..., 0] - top[..., 1] > 20.0).permute(0, 2, 1).reshape(-1, heads, 1).expand(-1, -1, hd).reshape(-1, heads * hd).cuda()
    print(f"queries with a clear maximum: {keep.float().mean().item():.4f}")
    assert keep.float().mean().item() > 0.97
    _check_attention(op, f"hiera attention, scores ~{pre:.0e}", got[keep], ref[keep], 0.03, 6e-3)


@pytest.mark.parametrize(*params("B,nq,nk,heads,hd,shared", [(3, 4096, 8, 8, 16, 0), (5, 8, 8, 8, 32, 0), (4, 8, 4096, 8, 16, 0), (4, 8, 4096, 8, 16, 1)]))
def test_dec_attention(gpu_lib, op, B, nq, nk, heads, hd, shared):
    g = torch.Generator().manual_seed(nq + nk)
    C_ = heads * hd
    q = torch.randn(B, nq, C_, generator=g)
    k = torch.randn(1 if shared else B, nk, C_, generator=g)
    v = torch.randn(1 if shared else B, nk, C_, generator=g)
    qq = q.view(B, nq, heads, hd).transpose(1, 2).double()
    kk = k.expand(B, -1, -1).reshape(B, nk, heads, hd).transpose(1, 2).double()
    vv = v.expand(B, -1, -1).reshape(B, nk, heads, hd).transpose(1, 2).double()
    ref = (torch.softmax(qq @ kk.transpose(-1, -2) / hd ** 0.5, -1) @ vv).transpose(1, 2).reshape(B, nq, C_)
    out = torch.zeros(B, nq, C_, dtype=torch.int16, device="cuda")
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    with operand_type(gpu_lib, op):
        kcall(gpu_lib, gpu_lib.saber_k_dec_attention(ptr(qd), ptr(kd), ptr(vd), ptr(out), B, nq, nk, heads, hd, shared, None))
    check_bound(op, "dec attention max abs", amax(from_dev(out, op).double() - ref), 0.02, bound16(op, 0.02, amax(ref)), sep_maxabs(ref))


@pytest.mark.parametrize("crop", [(0, 0, 1024, 1024), (100, 50, 597, 400), (700, 724, 300, 300), (10, 20, 200, 100)])
def test_mask_post(gpu_lib, crop):
    x0, y0, cw, ch = crop
    H = W = 1024
    g = torch.Generator().manual_seed(cw)
    n = 5
    low = F.interpolate(torch.randn(n, 1, 16, 16, generator=g) * 4, size=(256, 256), mode="bicubic")[:, 0].contiguous()
    low[4] = -5.0  # empty mask
    full = F.interpolate(low[:, None], size=(ch, cw), mode="bilinear", align_corners=False)[:, 0]
    thr, off = 0.0, 0.7
    ref_mask = torch.zeros(n, H, W, dtype=torch.bool)
    ref_mask[:, y0:y0 + ch, x0:x0 + cw] = full > thr
    bits = torch.zeros(n, H, W // 32, dtype=torch.int32, device="cuda")
    stats = torch.zeros(n, 8, dtype=torch.int32, device="cuda")
    low_d = low.cuda()
    kcall(gpu_lib, gpu_lib.saber_k_mask_post(ptr(low_d), n, x0, y0, cw, ch, H, W, thr, off, ptr(bits), ptr(stats), None))
    from saber_amd.engine import unpack_bits
    got = unpack_bits(bits, W)
    st = stats.cpu().numpy()
    for i in range(n):
        diff = np.logical_xor(got[i], ref_mask[i].numpy()).sum()
        assert diff <= 3, (i, diff)  # pixels whose logit sits within fp32 rounding of the threshold
        assert abs(int(st[i, 0]) - int(ref_mask[i].sum())) <= 3
        assert abs(int(st[i, 1]) - int((full[i] > thr + off).sum())) <= 3
        assert abs(int(st[i, 2]) - int((full[i] > thr - off).sum())) <= 3
        assert int(st[i, 0]) == int(got[i].sum())
        if got[i].any():
            ys, xs = np.where(got[i])
            assert (st[i, 3], st[i, 4], st[i, 5], st[i, 6]) == (xs.min(), ys.min(), xs.max(), ys.max())
    assert st[4, 0] == 0 and st[4, 5] == -1


@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_prepare(gpu_lib, dtype):
    from oracle import saber_ref
    img = saber_ref.synthetic_slice(seed=0)
    if dtype == "u16":
        dev = torch.from_numpy(img).cuda()
        ref = saber_ref.prepare(img.astype(np.float32))
        dt = 0
    else:
        f = (img.astype(np.float32) - 30000.0) / 7.0
        dev = torch.from_numpy(f).cuda()
        ref = saber_ref.prepare(f)
        dt = 1
    out = torch.zeros(1024, 1024, device="cuda")
    ws = torch.zeros(4, 1024, 1024, device="cuda")
    mm = torch.zeros(2, dtype=torch.int32, device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_prepare(ptr(dev), dt, 1024, 1024, ptr(out), ptr(ws), ptr(mm), None))
    err = np.abs(out.cpu().numpy() - ref).max()
    assert err < 2e-4, err
    assert out.min().item() == 0.0 and abs(out.max().item() - 1.0) < 1e-6


def test_perm_index_is_window_contiguous(lib):
    # every Hiera-L window is a contiguous, aligned run of rows; 2x2 pooling groups are 4 consecutive rows
    for stage, win in ((0, 8), (1, 4), (2, 16), (3, 8)):
        g = 256 >> stage
        idx = np.array([[lib.saber_k_perm_index(y, x, stage) for x in range(g)] for y in range(g)])
        assert sorted(idx.ravel().tolist()) == list(range(g * g))
        for wy in range(0, g, win):
            for wx in range(0, g, win):
                w = idx[wy:wy + win, wx:wx + win].ravel()
                assert w.max() - w.min() == win * win - 1 and w.min() % (win * win) == 0
        for y in range(0, g if stage < 3 else 0, 2):  # no pooling happens out of the last stage
            for x in range(0, g, 2):
                q = idx[y:y + 2, x:x + 2].ravel()
                assert q.tolist() == list(range(q[0], q[0] + 4)) and q[0] % 4 == 0


@pytest.mark.parametrize(*params("M,N,K,act,use_res", [
    (32768, 576, 576, 0, True),      # stage-2 proj: fp32 + residual fast epilogue of the persistent direct-to-LDS kernel
    (32768, 2304, 576, 1, False),    # stage-2 fc1: 16-bit + GELU epilogue (M N >= 2^26: the p256s kernel on W packed per K-step)
    (65536, 432, 144, 0, False),     # stage-0 qkv: K = 144 on zero-padded weight rows (engine upload layout)
    (70000, 288, 1152, 0, True),     # ragged M, N not a multiple of the 128 tile
]))
def test_gemm_direct_to_lds(gpu_lib, op, M, N, K, act, use_res):
    """Shapes of the Hiera blocks (the direct-to-LDS kernels every Hiera block runs); torch fp64 on the GPU is the reference."""
    g = torch.Generator(device="cuda").manual_seed(M + N)
    Kp = (K + 63) // 64 * 64
    A = torch.randn(M, K, device="cuda", generator=g).to(DTYPE[op])
    W = torch.zeros(N, Kp, device="cuda", dtype=DTYPE[op])
    W[:, :K] = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(DTYPE[op])
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g) if use_res else None
    ref = A.double() @ W[:, :K].double().T + bias.double()
    if act == 1:
        ref = F.gelu(ref)
    if use_res:
        ref = ref + res.double()
    with operand_type(gpu_lib, op):
        if use_res:
            out = torch.zeros(M, N, device="cuda")
            kcall(gpu_lib, gpu_lib.saber_k_gemm_ld(ptr(A), K, ptr(W), Kp, 1, ptr(bias), ptr(res), ptr(out), None, M, N, K, act, None))
            check_bound(op, "fp32 out (abs)", amax(out.double() - ref), 2e-4)
        else:
            out = torch.zeros(M, N, device="cuda", dtype=DTYPE[op])
            kcall(gpu_lib, gpu_lib.saber_k_gemm_ld(ptr(A), K, ptr(W), Kp, 1, ptr(bias), None, None, ptr(out), M, N, K, act, None))
            rel = lambda t: ((t - ref).abs() / (ref.abs() + 1.0)).max().item()
            # one 16-bit rounding of the output (+ the 2.6e-5 GELU fit)
            check_bound(op, "16-bit out, |err| / (|ref| + 1)", rel(out.double()), 2.0 ** -8, 2.0 ** -11, rel(rnd(ref, "bf16").double()))


def _dec_inputs(P, seed, op="bf16"):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, device="cuda", generator=g) * scale)
    X = r(P, 4096, 256).to(DTYPE[op])
    pe = r(4096, 256).to(DTYPE[op])
    return g, r, X, pe


def _blockdiag_pe_scores(tproj, pproj, scale):
    """scale * sum_i tproj[p, t, 16h + i] * pproj[n, 16h + i] -> [P, 64 = 8h + t, 4096] (the positional term of a folded attention)"""
    P = tproj.shape[0]
    tp = tproj.double().view(P, 8, 8, 16).permute(0, 2, 1, 3)          # [p][h][t][i]
    pp = pproj.double().view(4096, 8, 16)                              # [n][h][i]
    return scale * torch.einsum("phti,nhi->phtn", tp, pp).reshape(P, 64, 4096)


def i2t_inputs(P, shared, seed, op="bf16"):
    """operands of saber_k_dec_i2t in the operand type `op`"""
    g, r, X, pe = _dec_inputs(1 if shared else P, seed, op)
    T = DTYPE[op]
    return dict(X=X, Kt=r(P, 64, 256, scale=0.08).to(T), peq=r(4096, 128, scale=1.0).to(T), tk=r(P * 8, 128, scale=1.0), kscale=0.3, cb=r(P, 64),
                VtT=r(P, 256, 64, scale=0.5).to(T), bo=r(256), gamma=1.0 + 0.1 * r(256), beta=0.1 * r(256), P=P, shared=shared, op=op)


def i2t_launch(lib, d, X=None, out=None):
    X = d["X"] if X is None else X
    out = torch.zeros(d["P"], 4096, 256, device="cuda", dtype=DTYPE[d["op"]]) if out is None else out
    with operand_type(lib, d["op"]):
        kcall(lib, lib.saber_k_dec_i2t(ptr(X), 0 if d["shared"] else 4096 * 256, ptr(d["peq"]), ptr(d["Kt"]), ptr(d["tk"]), d["kscale"], ptr(d["cb"]),
                                       ptr(d["VtT"]), ptr(d["bo"]), ptr(d["gamma"]), ptr(d["beta"]), 1e-5, ptr(out), d["P"], None))
    return out


def i2t_ref(d, n=None):
    """out = LN(x + softmax_per_head(x Kt^T + kscale blockdiag(tk) peq^T + cb) Vt + bo) in fp64 for the first n prompts; scores live in the
    exp2 domain; the kernel rounds the scaled projection tk and the softmax weights P to the operand type for its MFMAs"""
    P = d["P"] if n is None else n
    T = DTYPE[d["op"]]
    Xd = d["X"].double().expand(d["P"], -1, -1)[:P]
    tkb = (d["tk"] * d["kscale"]).to(T).view(d["P"], 8, 128)[:P]
    S = Xd @ d["Kt"][:P].double().transpose(1, 2) + _blockdiag_pe_scores(tkb, d["peq"], 1.0).transpose(1, 2) + d["cb"][:P].double()[:, None, :]
    Pm = torch.softmax(S.view(P, 4096, 8, 8) * np.log(2.0), dim=-1).view(P, 4096, 64)
    Y = Pm.to(T).double() @ d["VtT"][:P].double().transpose(1, 2)
    return F.layer_norm(Xd + Y + d["bo"].double(), (256,), d["gamma"].double(), d["beta"].double(), 1e-5)


def check_i2t(op, what, got, ref):
    # 16-bit output of O(1..4) LayerNorm values: one bf16 ulp is 2^-7 at magnitude 2..4
    check_bound(op, f"{what} max abs", amax(got - ref), 0.04, bound16(op, 0.04, amax(ref)), sep_maxabs(ref))
    check_bound(op, f"{what} rms", (got - ref).pow(2).mean().sqrt().item(), 4e-3, 4e-3 / 8, sep_rms(ref))


@pytest.mark.parametrize(*params("P,shared", [(3, False), (2, True), (70, False)]))
def test_dec_i2t(gpu_lib, op, P, shared):
    """Folded image->token attention + residual + LayerNorm (dec_i2t_kernel) against the plain formula in fp64 (i2t_ref)"""
    d = i2t_inputs(P, shared, 11 + P, op)
    out = i2t_launch(gpu_lib, d)
    check_i2t(op, "dec_i2t", out.double(), i2t_ref(d))


def t2i_inputs(P, shared, seed, op="bf16", split=1):
    g, r, X, pe = _dec_inputs(1 if shared else P, seed, op)
    T = DTYPE[op]
    return dict(X=X, Qt=r(P, 64, 256, scale=0.05).to(T), pek=r(4096, 128, scale=1.0).to(T), tq=r(P * 8, 128, scale=1.0), qscale=0.3,
                Wv=(r(128, 256) / 16).to(T), bv=r(128), part=torch.zeros(P * split * 64 * 256, device="cuda"),
                ml=torch.zeros(P * split * 64 * 2, device="cuda"), P=P, split=split, shared=shared, op=op)


def t2i_launch(lib, d):
    out = torch.zeros(d["P"], 8, 128, device="cuda", dtype=DTYPE[d["op"]])
    with operand_type(lib, d["op"]):
        kcall(lib, lib.saber_k_dec_t2i(ptr(d["X"]), 0 if d["shared"] else 4096 * 256, ptr(d["pek"]), ptr(d["Qt"]), ptr(d["tq"]), d["qscale"], ptr(d["part"]),
                                       ptr(d["ml"]), d["P"], d["split"], ptr(d["Wv"]), ptr(d["bv"]), ptr(out), None))
    return out


def t2i_ref(d):
    """out[p][t][16h+i] = Wv[16h+i] . (sum_n softmax_n(Qt[8h+t] . x_n + qscale tq[h,t] . pek_n[h]) x_n) + bv; the kernel rounds the scaled
    projection tq to the operand type (P is rounded before the PV MFMA: within the bound)"""
    P = d["P"]
    Xd = d["X"].double().expand(P, -1, -1)
    tqb = (d["tq"] * d["qscale"]).to(DTYPE[d["op"]]).view(P, 8, 128)
    S = d["Qt"].double() @ Xd.transpose(1, 2) + _blockdiag_pe_scores(tqb, d["pek"], 1.0)   # [P, 64, 4096], exp2 domain
    Z = (torch.softmax(S * np.log(2.0), dim=-1) @ Xd).view(P, 8, 8, 256)                    # [p][h][t][256]
    return torch.einsum("phtd,hid->pthi", Z, d["Wv"].double().view(8, 16, 256)).reshape(P, 8, 128) + d["bv"].double()


def check_t2i(op, what, got, ref):
    scale = amax(ref)
    # P is rounded to the operand type before the PV MFMA, output stored as 16-bit
    check_bound(op, f"{what} max abs / max|ref|", amax(got - ref) / scale, 0.02, bound16(op, 0.02, 1.0), sep_maxabs(ref) / scale)


@pytest.mark.parametrize(*params("P,split,shared", [(3, 1, False), (2, 4, True), (5, 8, False)]))
def test_dec_t2i(gpu_lib, op, P, split, shared):
    """Folded token->image attention (dec_t2i_kernel + finish) against t2i_ref in fp64"""
    d = t2i_inputs(P, shared, 5 + P, op, split)
    out = t2i_launch(gpu_lib, d)
    check_t2i(op, "dec_t2i", out.double(), t2i_ref(d))


def _race_screen(lib, op):
    """Race screen for the kernels that order LDS-DMA traffic by hand (counted vmcnt + raw barriers): the same launch repeated must be
    bit-identical every time (a read that overtakes its DMA shows up as run-to-run differences long before it fails a tolerance)."""
    g = torch.Generator().manual_seed(99)
    # staggered 256x256 GEMM (its normal route: >= 1024 tiles, N >= 1024)
    M, N, K = 256 * 130, 2304, 576
    Ad = to_dev(torch.randn(M, K, generator=g), op)
    Wd = to_dev(torch.randn(N, K, generator=g) / K ** 0.5, op)
    bias = torch.randn(N, generator=g).cuda()
    outs = []
    with operand_type(lib, op):
        for _ in range(6):
            o = torch.zeros(M, N, dtype=torch.int16, device="cuda")
            kcall(lib, lib.saber_k_gemm(ptr(Ad), ptr(Wd), ptr(bias), None, None, ptr(o), M, N, K, 1, 0, 0, 0, 0, None))
            outs.append(o)
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    # streaming global attention and the 256-key window kernel
    for nw, nk, heads in ((5, 4096, 8), (70, 256, 8)):
        qd = to_dev(torch.randn(nw * nk, 3 * heads * 72, generator=g) * 1.5, op)
        outs = []
        with operand_type(lib, op):
            for _ in range(6):
                o = torch.zeros(nw * nk, heads * 72, dtype=torch.int16, device="cuda")
                kcall(lib, lib.saber_k_hiera_attention(ptr(qd), ptr(o), nw, nk, heads, 0, None))
                outs.append(o)
        assert all(torch.equal(outs[0], o) for o in outs[1:])
    # decoder streaming kernels
    P = 300
    gg, r, X, pe = _dec_inputs(P, 123, op)
    T = DTYPE[op]
    Kt = r(P, 64, 256, scale=0.08).to(T); peq = r(4096, 128).to(T); tk = r(P * 8, 128); cb = r(P, 64)
    VtT = r(P, 256, 64, scale=0.5).to(T); bo, gamma, beta = r(256), 1.0 + 0.1 * r(256), 0.1 * r(256)
    Wv = (r(128, 256) / 16).to(T); bv = r(128)
    part = torch.zeros(P * 64 * 256, device="cuda"); ml = torch.zeros(P * 64 * 2, device="cuda")
    o1, o2 = [], []
    with operand_type(lib, op):
        for _ in range(4):
            a = torch.zeros(P, 4096, 256, device="cuda", dtype=T)
            kcall(lib, lib.saber_k_dec_i2t(ptr(X), 4096 * 256, ptr(peq), ptr(Kt), ptr(tk), 0.3, ptr(cb), ptr(VtT), ptr(bo), ptr(gamma), ptr(beta), 1e-5, ptr(a), P, None))
            b = torch.zeros(P, 8, 128, device="cuda", dtype=T)
            kcall(lib, lib.saber_k_dec_t2i(ptr(X), 4096 * 256, ptr(peq), ptr(Kt), ptr(tk), 0.3, ptr(part), ptr(ml), P, 1, ptr(Wv), ptr(bv), ptr(b), None))
            o1.append(a); o2.append(b)
    assert all(torch.equal(o1[0], o) for o in o1[1:]) and all(torch.equal(o2[0], o) for o in o2[1:])


def test_hand_synchronised_kernels_are_run_to_run_identical(gpu_lib):
    _race_screen(gpu_lib, "bf16")


@pytest.mark.parametrize("op", OPS)
def test_hand_synchronised_one_wave_and_rowln_kernels_are_run_to_run_identical(gpu_lib, op):
    """the same screen for gemm_rowln_kernel<2,4> (N = 576) and the two one-wave-per-SIMD decoder kernels dec_t2i_w1 (forced, split 1) and
    dec_i2t_w1 (P >= 512): the fp16 builds of these carry different spills and register allocations than the bf16 ones"""
    M, N, K = 128 * 300 + 17, 576, 2304
    g = torch.Generator(device="cuda").manual_seed(7)
    A = (torch.randn(M, K, device="cuda", generator=g) * 0.7).to(DTYPE[op])
    W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(DTYPE[op])
    bias, gamma, beta = torch.randn(N, device="cuda", generator=g), torch.rand(N, device="cuda", generator=g) + 0.5, torch.randn(N, device="cuda", generator=g) * 0.1
    res = torch.randn(M, N, device="cuda", generator=g)
    outs = []
    with operand_type(gpu_lib, op):
        for _ in range(4):
            y = res.clone()
            yb = torch.zeros(M, N, dtype=DTYPE[op], device="cuda")
            ln = torch.zeros(M, N, dtype=DTYPE[op], device="cuda")
            kcall(gpu_lib, gpu_lib.saber_k_gemm_rowln(ptr(A), K, ptr(W), K, ptr(bias), ptr(y), ptr(y), ptr(yb), ptr(gamma), ptr(beta), 1e-6, ptr(ln), M, N, K, None))
            outs.append((y, yb, ln))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o)), "gemm_rowln<2,4>"
    d = t2i_inputs(300, False, 31, op)
    gpu_lib.saber_k_set_debug(0x10000000)
    try:
        o = [t2i_launch(gpu_lib, d) for _ in range(4)]
    finally:
        gpu_lib.saber_k_set_debug(0)
    assert all(torch.equal(o[0], x) for x in o[1:]), "dec_t2i_w1"
    d = i2t_inputs(520, False, 37, op)
    o = [i2t_launch(gpu_lib, d) for _ in range(4)]
    assert all(torch.equal(o[0], x) for x in o[1:]), "dec_i2t_w1"


def test_hand_synchronised_kernels_are_run_to_run_identical_fp16(gpu_lib):
    _race_screen(gpu_lib, "fp16")


# gemm_rowln (csrc/gemm_rowln.hip launch_gemm_rowln) configuration by N: 576 -> gemm_rowln_kernel<2,4> (128-row tiles),
# 288 -> <4,2> (256-row tiles), 144 -> <8,1> (512-row tiles)
ROWLN_CFG = {576: "rowln24", 288: "rowln42", 144: "rowln81"}


def _rowln_run(lib, op, M, N, K, A, Wf, bias, res, gamma, beta, with_bf=True):
    Kp = (K + 63) // 64 * 64
    Wp = torch.zeros(N, Kp, dtype=DTYPE[op], device="cuda")
    Wp[:, :K] = Wf
    out = (res.clone() if res is not None else torch.zeros(M, N, device="cuda"))      # in place: res aliases out_f32, as the engine's residual stream does
    out_bf = torch.zeros(M, N, dtype=DTYPE[op], device="cuda") if with_bf else None
    ln_out = torch.zeros(M, N, dtype=DTYPE[op], device="cuda")
    with operand_type(lib, op):
        kcall(lib, lib.saber_k_gemm_rowln(ptr(A), K, ptr(Wp), Kp, ptr(bias), ptr(out) if res is not None else None, ptr(out), ptr(out_bf),
                                          ptr(gamma), ptr(beta), 1e-6, ptr(ln_out), M, N, K, None))
    return out, out_bf, ln_out


@pytest.mark.parametrize(*params("M,N,K,with_res,with_bf", [(4096, 576, 576, True, False), (4096 + 70, 576, 2304, True, True), (16384, 288, 1152, True, False),
                                                            (2048 + 300, 288, 288, False, True), (65536, 144, 144, True, False), (4096 + 33, 144, 576, True, True),
                                                            (128 * 356 + 17, 576, 576, True, False)]))      # 357 tiles on 256 workgroups: uneven walks, the short ones start late
def test_gemm_rowln(gpu_lib, op, M, N, K, with_res, with_bf):
    """residual GEMM + the LayerNorm that follows it in one kernel (gemm_rowln.hip): y against fp64 on the same 16-bit operands,
    the normalised 16-bit rows against LayerNorm of the kernel's own y (<= 1 ulp of the type, almost all exact) and of the fp64 y"""
    g = torch.Generator().manual_seed(M + N + K)
    A = (torch.randn(M, K, generator=g) * 0.7).to(DTYPE[op])
    Wf = (torch.randn(N, K, generator=g) / K ** 0.5).to(DTYPE[op])
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g) * 2 + 0.5 if with_res else None
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.1
    Ad, Wd, bd, gd, bed = A.cuda(), Wf.cuda(), bias.cuda(), gamma.cuda(), beta.cuda()
    print(ROWLN_CFG[N])
    out, out_bf, ln_out = _rowln_run(gpu_lib, op, M, N, K, Ad, Wd, bd, res.cuda() if with_res else None, gd, bed, with_bf)
    ref = Ad.double() @ Wd.double().T + bd.double() + (res.cuda().double() if with_res else 0.0)
    y = out
    check_bound(op, f"{ROWLN_CFG[N]} y (fp32) / max|y|", amax(y.double() - ref) / amax(ref), 2e-5)
    if with_bf:
        assert torch.equal(out_bf.float(), rnd(y, op))
    ln_self = F.layer_norm(y.cpu(), (N,), gamma, beta, 1e-6)
    got = ln_out.cpu().float()
    d = (got - rnd(ln_self, op)).abs()
    ulp_scale = ln_self.abs().clamp(min=1e-3)
    ulp = ulp_scale * (2.0 ** -7 if op == "bf16" else 2.0 ** -10)           # one ulp of the type (an upper bound)
    e_ulp = float((d / ulp).max())
    print(f"{ROWLN_CFG[N]} LayerNorm rows [{op}]: max |d| / ulp {e_ulp:.3f} (bound 1); one bf16 rounding of the rows "
          f"{float(((rnd(ln_self, 'bf16') - ln_self).abs() / ulp).max()):.1f} fp16 ulps")
    assert (d <= ulp).all(), e_ulp
    assert (d > 0).float().mean().item() < 2e-3         # rounding flips only
    ln_ref = F.layer_norm(ref, (N,), gd.double(), bed.double(), 1e-6).cpu()
    check_bound(op, f"{ROWLN_CFG[N]} rows vs LayerNorm of the fp64 y", amax(got.double() - ln_ref), 0.05, bound16(op, 0.05, amax(ln_ref)), sep_maxabs(ln_ref))


@pytest.mark.parametrize("cfg,N,K", [("rowln24", 576, 576), ("rowln42", 288, 1152), ("rowln81", 144, 288)])
@pytest.mark.parametrize("case", ["overflow", "large"])
def test_gemm_rowln_fp16_range(gpu_lib, cfg, N, K, case):
    """fp16 range edges of gemm_rowln, each configuration: 'large' - a residual stream of |y| ~ 3e4 (inside the range: the 16-bit copy of y
    and the LayerNorm rows must be finite and as exact as at O(1)); 'overflow' - every third column beyond 65 520 (the 16-bit copy of y
    +-inf there and RNE elsewhere, y in fp32 exact, the LayerNorm of the fp32 rows finite)"""
    assert ROWLN_CFG[N] == cfg
    M = 4096 + 45
    g = torch.Generator(device="cuda").manual_seed(N + K)
    A = (torch.randn(M, K, device="cuda", generator=g) * 0.7).to(torch.float16)
    Wf = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(torch.float16)
    bias = torch.randn(N, device="cuda", generator=g)
    gamma, beta = torch.rand(N, device="cuda", generator=g) + 0.5, torch.randn(N, device="cuda", generator=g) * 0.1
    if case == "large":
        res = (torch.rand(M, N, device="cuda", generator=g) * 2 - 1) * 3.2e4
    else:
        res = torch.randn(M, N, device="cuda", generator=g)
        res[:, ::3] *= 6.0e4
    out, out_bf, ln_out = _rowln_run(gpu_lib, "fp16", M, N, K, A, Wf, bias, res, gamma, beta)
    ref = A.double() @ Wf.double().T + bias.double() + res.double()
    check_bound("fp16", f"{cfg} {case}: y (fp32) / max|y|", amax(out.double() - ref) / amax(ref), 2e-5)
    if case == "large":
        print(f"{cfg}: max |y| {amax(ref):.3e}")
        assert amax(ref) < 65504 and torch.isfinite(out_bf).all()
        assert torch.equal(out_bf.float(), rnd(out, "fp16"))
    else:
        _check_fp16_overflow(f"{cfg} out_bf16 overflow", ref, out_bf.double(), out.double())
    ln_ref = F.layer_norm(ref, (N,), gamma.double(), beta.double(), 1e-6)
    got = ln_out.double()
    assert torch.isfinite(got).all()
    check_bound("fp16", f"{cfg} {case}: rows vs LayerNorm of the fp64 y", amax(got - ln_ref), 0.05, bound16("fp16", 0.05, amax(ln_ref)), sep_maxabs(ln_ref))


def _rowln_late_start(lib, op):
    """gemm_rowln_kernel starts the workgroups with the shorter tile walk late (timing only): same bits with the late start switched off
    (saber_k_set_debug(32768)), on a problem whose tile count (357) is not a multiple of the grid (256)"""
    M, N, K = 128 * 356 + 17, 576, 2304
    g = torch.Generator().manual_seed(5)
    A = to_dev(torch.randn(M, K, generator=g) * 0.7, op)
    W = to_dev(torch.randn(N, K, generator=g) / K ** 0.5, op)
    bias, gamma, beta = torch.randn(N, generator=g).cuda(), (torch.rand(N, generator=g) + 0.5).cuda(), (torch.randn(N, generator=g) * 0.1).cuda()
    res = (torch.randn(M, N, generator=g) * 2).cuda()
    outs = []
    for flag in (0, 32768, 0):
        lib.saber_k_set_debug(flag)
        try:
            y = res.clone()
            ln = torch.zeros(M, N, dtype=torch.uint16, device="cuda")
            with operand_type(lib, op):
                kcall(lib, lib.saber_k_gemm_rowln(ptr(A), K, ptr(W), K, ptr(bias), ptr(y), ptr(y), None, ptr(gamma), ptr(beta), 1e-6, ptr(ln), M, N, K, None))
        finally:
            lib.saber_k_set_debug(0)
        outs.append((y, ln))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])


def test_gemm_rowln_late_start_changes_nothing(gpu_lib):
    _rowln_late_start(gpu_lib, "bf16")


def test_gemm_rowln_late_start_changes_nothing_fp16(gpu_lib):
    _rowln_late_start(gpu_lib, "fp16")
