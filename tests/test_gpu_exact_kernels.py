"""GPU: the exact-precision (fp32) kernels of csrc/exact.hip one by one, through the kernel-level entry points saber_k_xg_* (include/saber_amd_kernels.h),
against torch in fp64 on the GPU evaluated on the same fp32 operands the kernel gets.

Routes.  xg_gemm, xg_attn and xg_layernorm choose among 14 kernels by shape, head dimension and pointer alignment; the *_route functions below
restate each dispatcher's choice, every case asserts the route it is predicted to take, and test_every_route_has_a_case fails on the day a
route is added to ROUTES without a case.  Cases are built so that a structural bug (a dropped key or k, a wrong tile edge, row mapping,
slab offset or segment merge) moves the result by O(1), not by one rounding.

Bounds come from the reference alone, never from the kernel:
  E_f32 = max over the case of |torch fp32 evaluation of the same formula - fp64 reference| (TF32 off, cudnn off).  For the GEMMs the fp32
          evaluation is a K-sequential accumulation (v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered fmaf chain, so every output of xg_gemm*
          is one fp32 chain over a permuted k order; a blocked library sum would understate that spread).
  GEMM:   4 E_f32 (two draws of the maximum over >= 1e5 outputs differ by < 2x; a fused or unfused reference chain, another 2x), and every
          element inside the rigorous fp32 bound  L gamma_{K+2} (|A| |W|^T + |bias|) + u |res| + u |out| + E_act,  gamma_n = n u / (1 - n u),
          u = 2^-24, L the activation's Lipschitz constant (1.13 GELU, 1/4 sigmoid), u |out| the rounding of the stored sum and E_act torch's own
          fp32-vs-fp64 error of the activation on the fp64 pre-activations rounded to fp32.
  others: 8 E_f32 (attention, LayerNorm, add, add_slot, mask_hidden, mask_dot: another summation order and an online softmax, as bound_of in
          test_gpu_decoder_head.py).
Separation: in every case the bound is below the error of the same formula on bf16-rounded operands (a route that fell back to 16-bit
arithmetic fails), and in GELU cases below max |tanh-GELU - erf-GELU| over the case's pre-activations (x_gelu is the erf form).

Every output buffer starts filled with the NaN canary of test_gpu_decoder_head: every element of the result must have been written and every
other element of the buffer (padding columns ldc > N / ldo > heads * hd, the guard behind it) must still hold the canary.  Each case prints
err / bound; the largest ratio per kernel family on an MI355X is recorded in README.md."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_decoder_head import CANARY, perm_grid, to_engine_order

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LIP = {0: 1.0, 1: 1.13, 2: 1.0, 3: 0.25}            # act: 0 none, 1 GELU(erf), 2 ReLU, 3 sigmoid (csrc/kernels.h ACT_*)
GUARD = 256                                          # canary floats behind every output
SLAB_ROWS = 65535 * 128                              # rows of one xg_gemm_kernel launch (gridDim.y <= 65535 tiles of 128 rows)
RATIOS = {}                                          # family -> largest err / bound of this run


def p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * off)


def kcall(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()
    torch.cuda.synchronize()


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def canary_buf(n):
    return torch.full((n + GUARD,), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)


def check_written(buf, view, what):
    """every element of `view` (a strided view into `buf`) written, every other element of buf still the canary"""
    bits = buf.view(torch.int32)
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
    inside.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
    assert not (bits[inside] == CANARY).any(), (what, "result elements left unwritten")
    assert (bits[~inside] == CANARY).all(), (what, "elements outside the result written (padding columns or beyond the end)")


def gelu_tanh(x):
    return F.gelu(x, approximate="tanh")


def act_fn(act, x):
    if act == 1:
        return F.gelu(x)
    if act == 2:
        return torch.relu(x)
    if act == 3:
        return torch.sigmoid(x)
    return x


def record(family, what, err, bound, sep, tanh_gap=None):
    """print err / bound and assert the separations and the bound"""
    r = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)
    extra = "" if tanh_gap is None else f", |tanh - erf GELU| {tanh_gap:.3e}"
    print(f"{family} {what}: err {err:.3e} / bound {bound:.3e} = {r:.3f} (bf16 operands {sep:.3e}{extra})")
    assert bound < sep, (what, "the bound does not tell fp32 from bf16 operands", bound, sep)
    if tanh_gap is not None:
        assert bound < tanh_gap, (what, "the bound does not tell the erf GELU from the tanh form", bound, tanh_gap)
    assert err <= bound, (what, err, bound)
    return r


def amax(t):
    return t.abs().max().item()


@pytest.fixture(scope="module", autouse=True)
def fp32_references():
    assert not torch.backends.cuda.matmul.allow_tf32, "the fp32 reference must not use TF32"
    with torch.backends.cudnn.flags(enabled=False), torch.no_grad():
        yield
    print("largest err / bound per kernel family:", {k: round(v, 3) for k, v in sorted(RATIOS.items())})


# ------------------------------------------------------------------------------------------------ routes
ROUTES = (
    "gemm2<128> one tile", "gemm2<128> persistent", "gemm2<64> one tile", "gemm2<64> persistent", "gemm unaligned", "gemm unaligned slabs",
    "attn fewq mfma", "attn fewq valu", "attn fewk", "attn mfma<56>", "attn mfma<72>", "attn mfma<96>",
    "attn generic<16>", "attn generic<32>", "attn generic<56>", "attn generic<72>", "attn generic<96>",
    "ln4<16,1>", "ln4<64,1>", "ln4<64,1> row_valid", "ln4<64,5>", "ln4<64,5> row_valid", "ln general", "ln general row_valid",
    "add", "add_slot4", "add_slot scalar", "mask_hidden", "mask_dot",
)


def al(*xs):
    return all(x % 4 == 0 for x in xs)


def gemm_route(g):
    """xg_gemm (csrc/exact.hip): 16-byte rows -> xg_gemm2_kernel<BN>, one tile per workgroup or persistent over row tiles; else xg_gemm_kernel in
    slabs of 65 535 row tiles.  Offsets are in floats from a 256-byte aligned allocation."""
    M, N, K, B = g["M"], g["N"], g["K"], g.get("batch", 1)
    vec = al(g["lda"], g["ldw"], g.get("sA", 0), g.get("sW", 0), K, g.get("a_off", 0), 0) and (not g.get("a2_mod") or al(g["lda2"]))
    gy = -(-M // 128)
    if vec:
        bn = 128 if (N > 64 and not (K <= 128 and N <= 256)) else 64
        gx = -(-N // bn)
        ny = max(1, n_cu() * (3 if bn == 128 else 4) // (gx * B))
        if gy < 8 * ny and gy <= 65535:
            ny = gy
        ny = min(ny, gy, 65535)
        return f"gemm2<{bn}> " + ("one tile" if ny == gy else "persistent")
    return "gemm unaligned slabs" if gy > 65535 else "gemm unaligned"


def attn_route(a):
    """xg_attn (csrc/exact.hip), in its dispatch order"""
    hd, nq, nk, H = a["hd"], a["nq"], a["nk"], a["heads"]
    L = attn_layout(a)
    qp, km = a.get("qpool", 0), a.get("kmask") is not None
    if hd == 16 and nq <= 16 and nk >= 1024 and not qp and not km and al(L["ldk"], L["ldv"], L["k_bs"], L["v_bs"], L["k_off"], L["v_off"]):
        return "attn fewq mfma" if al(L["ldq"], L["q_bs"], L["q_off"]) else "attn fewq valu"
    if hd == 16 and H == 8 and nk <= 16 and nq >= 256 and not qp and not km and al(L["ldq"], L["ldo"], L["q_bs"], L["o_bs"], L["q_off"], L["o_off"]):
        return "attn fewk"
    if hd in (56, 72, 96) and al(L["ldk"], L["ldv"], L["ldo"], L["k_bs"], L["v_bs"], L["o_bs"], L["k_off"], L["v_off"], L["o_off"]):
        return f"attn mfma<{hd}>"
    return f"attn generic<{hd}>"


def ln_route(c):
    C_, rv, aligned = c["C"], c.get("valid_mod", 0) > 0, c.get("x_off", 0) == 0
    if aligned and C_ % 4 == 0 and C_ == 64 and not rv:
        return "ln4<16,1>"
    if aligned and C_ % 4 == 0 and C_ <= 256:
        return "ln4<64,1>" + (" row_valid" if rv else "")
    if aligned and C_ % 4 == 0 and C_ <= 1280:
        return "ln4<64,5>" + (" row_valid" if rv else "")
    return "ln general" + (" row_valid" if rv else "")


def add_slot_route(c):
    return "add_slot4" if al(c["C"], c["stride"], c.get("off4", 0)) else "add_slot scalar"


# ------------------------------------------------------------------------------------------------ GEMM
def persistent_m(N, K):
    """the smallest M whose row tiles the gemm2 kernel walks persistently (gy = 8 ny, the last tile one row)"""
    bn = 128 if (N > 64 and not (K <= 128 and N <= 256)) else 64
    ny = max(1, n_cu() * (3 if bn == 128 else 4) // -(-N // bn))
    return (8 * ny - 1) * 128 + 1


# name -> case.  Every case has >= 1e5 outputs (the 4 E_f32 argument).  tail: A[:, K-1] dominant (inside a partial last K step where K is not
# a multiple of 32 / 16); M, N ragged against the 128 x BN tiles everywhere.
GEMM_CASES = {
    "k_tail_gelu": dict(M=1000, N=300, K=200, lda=204, ldw=200, ldc=304, act=1, tail=True),
    "res_shift2": dict(M=1030, N=200, K=256, lda=256, ldw=260, ldc=200, res="shift", res_shift=2, ldres=204),
    "res_mod": dict(M=1500, N=96, K=64, lda=64, ldw=64, ldc=100, res="mod", res_mod=37, ldres=100, act=2),
    "a2_mod": dict(M=3001, N=128, K=60, lda=64, ldw=60, ldc=132, a2_mod=333, lda2=68, tail=True),
    "slot_res": dict(M=1700, N=128, K=64, lda=64, ldw=64, ldc=128, res="slot", res_rows_per=100, res_div=3, res_off=2, ldres=132),
    "slot_res_gelu_last": dict(M=1750, N=120, K=64, lda=64, ldw=64, ldc=124, res="slot", res_rows_per=250, res_div=2, res_off=1, ldres=128,
                               act=1, act_last=1),
    "hyper_batch4": dict(M=130, N=256, K=256, lda=8 * 256, sA=256, ldw=256, sW=256 * 256, sBias=256, ldc=256, sC=130 * 256, batch=4, act=2),
    "hyper_batch4_out": dict(M=800, N=32, K=256, lda=256, sA=800 * 256, ldw=256, sW=32 * 256, sBias=32, ldc=128, sC=32, batch=4),
    "pool4_128": dict(M=2052, N=288, K=144, lda=144, ldw=144, ldc=292, pool4=1, tail=True),
    "pool4_64": dict(M=8000, N=64, K=64, lda=68, ldw=64, ldc=64, pool4=1),
    "unaligned_base_sigmoid": dict(M=1100, N=100, K=64, lda=64, ldw=64, ldc=104, a_off=1, act=3, res="rows", ldres=100),
    "unaligned_lda_res_last_relu": dict(M=1100, N=100, K=64, lda=65, ldw=64, ldc=100, act=2, act_last=1, res="rows", ldres=104),
    "unaligned_k51_mod": dict(M=1203, N=90, K=51, lda=51, ldw=53, ldc=93, tail=True, res="mod", res_mod=5, res_shift=1, ldres=90),
    "unaligned_pool4": dict(M=6000, N=70, K=33, lda=33, ldw=33, ldc=71, pool4=1, tail=True),
    # the persistent walks (csrc/exact.hip: gy >= 8 ny); M depends on the CU count
    "persistent128_gelu_res": dict(M=None, N=288, K=36, lda=36, ldw=36, ldc=292, act=1, res="rows", ldres=288, tail=True),
    "persistent64_a2_slots": dict(M=None, N=256, K=64, lda=64, ldw=64, ldc=256, a2_mod=4096, lda2=64, res="slot", res_rows_per=4096, res_div=3,
                                  res_off=2, ldres=256),
    # the row slabs of xg_gemm_kernel: the second slab's A, C and residual offsets
    "slabs_res": dict(M=SLAB_ROWS + 1000, N=19, K=3, lda=3, ldw=3, ldc=21, res="rows", ldres=23, tail=True),
    "slabs_pool4": dict(M=SLAB_ROWS + 1000, N=19, K=3, lda=3, ldw=3, ldc=21, pool4=1, tail=True),
}
# act x act_last on the gemm2<64> route, with a residual (act_last only changes anything with one)
for _a in range(4):
    for _l in range(2):
        GEMM_CASES[f"act{_a}_last{_l}"] = dict(M=2050, N=60, K=52, lda=52, ldw=52, ldc=64, act=_a, act_last=_l, res="rows", ldres=60, tail=True)


def gemm_expected(name):
    """the route each case is written for"""
    if name.startswith("slabs"):
        return "gemm unaligned slabs"
    if name.startswith("unaligned"):
        return "gemm unaligned"
    if name.startswith("persistent"):
        return "gemm2<128> persistent" if name.startswith("persistent128") else "gemm2<64> persistent"
    return "gemm2<128> one tile" if name in ("k_tail_gelu", "res_shift2", "hyper_batch4", "pool4_128") else "gemm2<64> one tile"


def gemm_case(name):
    g = dict(GEMM_CASES[name])
    if g["M"] is None:
        g["M"] = persistent_m(g["N"], g["K"])
    g.setdefault("seed", sum(map(ord, name)))
    return g


def strided(flat, shape, stride, off):
    return flat.as_strided(shape, stride, off)


def run_gemm(lib, name):
    g = gemm_case(name)
    M, N, K, B = g["M"], g["N"], g["K"], g.get("batch", 1)
    act, act_last, pool4 = g.get("act", 0), g.get("act_last", 0), g.get("pool4", 0)
    lda, ldw, ldc, sA, sW, sBias, sC = g["lda"], g["ldw"], g["ldc"], g.get("sA", 0), g.get("sW", 0), g.get("sBias", 0), g.get("sC", 0)
    a_off = g.get("a_off", 0)
    Mo = M // 4 if pool4 else M
    assert Mo * N * B >= 100000, (name, "fewer than 1e5 outputs")
    route = gemm_route(g)
    assert route == gemm_expected(name), (name, route)
    print(f"\n{name}: M {M} N {N} K {K} batch {B} -> {route}")
    gen = torch.Generator(device="cuda").manual_seed(g["seed"])
    rn = lambda n, s=1.0: torch.randn(n, generator=gen, device="cuda") * s
    wscale = 1.0 / math.sqrt(K)
    A_flat = rn(a_off + (B - 1) * sA + (M - 1) * lda + K + 7)
    W_flat = rn((B - 1) * sW + (N - 1) * ldw + K + 7, wscale)
    b_flat = rn((B - 1) * sBias + N, 0.5)
    A = strided(A_flat, (B, M, K), (sA, lda, 1), a_off)
    W = strided(W_flat, (B, N, K), (sW, ldw, 1), 0)
    bias = strided(b_flat, (B, N), (sBias, 1), 0)
    if g.get("tail"):
        A[..., K - 1] = 4.0 + torch.rand(A.shape[:-1], generator=gen, device="cuda")      # a dominant term at k = K - 1
    A2_flat, Aop = None, A
    if g.get("a2_mod"):
        A2_flat = rn((g["a2_mod"] - 1) * g["lda2"] + K + 7)
        A2 = strided(A2_flat, (g["a2_mod"], K), (g["lda2"], 1), 0)
        Aop = A + A2[torch.arange(M, device="cuda") % g["a2_mod"]][None]          # the operand the kernel forms: one fp32 sum
    res_flat, R = None, None
    kind = g.get("res")
    rows = torch.arange(M, device="cuda")
    if kind:
        ldres = g["ldres"]
        if kind == "slot":
            rpp, div, off = g["res_rows_per"], g["res_div"], g["res_off"]
            n_pr = -(-M // rpp)
            n_slots = (n_pr - 1 + off) // div + 1
            stride = rpp * ldres + 12
            g["res_stride"] = stride
            res_flat = rn(n_slots * stride)
            base = ((rows // rpp + off) // div) * stride + (rows % rpp) * ldres
            assert n_pr % div != 0 and off > 0
        else:
            rr = rows >> g.get("res_shift", 0)
            if g.get("res_mod"):
                rr = rr % g["res_mod"]
            res_flat = rn((int(rr.max()) + 1) * ldres + 7)
            base = rr * ldres
        R = res_flat[base[:, None] + torch.arange(N, device="cuda")[None]]        # [M][N], shared by every batch entry
    C_flat = canary_buf((B - 1) * sC + (Mo - 1) * ldc + N)
    Cv = strided(C_flat, (B, Mo, N), (sC, ldc, 1), 0)
    kcall(lib, lib.saber_k_xg_gemm(p(A_flat, a_off), lda, sA, p(A2_flat), g.get("lda2", 0), g.get("a2_mod", 1), p(W_flat), ldw, sW, p(b_flat), sBias,
                                   p(res_flat), g.get("ldres", 0), g.get("res_shift", 0), g.get("res_mod", 0), g.get("res_rows_per", 0), g.get("res_stride", 0),
                                   g.get("res_div", 1), g.get("res_off", 0), p(C_flat), ldc, sC, M, N, K, act, act_last, pool4, B, None))
    check_written(C_flat, Cv, name)
    got = Cv.double()

    def epilogue(acc, bias_, R_):
        if pool4:
            return acc.view(B, Mo, 4, N).amax(2) + bias_[:, None]
        v = acc + bias_[:, None]
        if not act_last:
            v = act_fn(act, v)
        if R_ is not None:
            v = v + R_[None]
        return act_fn(act, v) if act_last else v

    # fp64 reference on the fp32 operands, and the pre-activations it feeds the activation
    acc64 = torch.matmul(Aop.double(), W.double().transpose(1, 2))
    ref = epilogue(acc64, bias.double(), None if R is None else R.double())
    pre = acc64 + bias.double()[:, None]
    if act_last and R is not None:
        pre = pre + R.double()[None]
    # fp32, K-sequential
    acc32 = torch.zeros(B, M, N, device="cuda")
    for k in range(K):
        acc32.addcmul_(Aop[:, :, k, None], W[:, None, :, k])
    e_f32 = amax(epilogue(acc32, bias, R).double() - ref)
    bound = 4 * e_f32
    # bf16 operands
    Ab, Wb = Aop.to(torch.bfloat16).double(), W.to(torch.bfloat16).double()
    sep = amax(epilogue(torch.matmul(Ab, Wb.transpose(1, 2)), bias.double(), None if R is None else R.double()) - ref)
    del Ab, Wb, acc32
    # rigorous per-element bound
    nu = (K + 2) * U
    absaw = torch.matmul(Aop.double().abs(), W.double().abs().transpose(1, 2))
    if pool4:
        absaw = absaw.view(B, Mo, 4, N).amax(2)
    rig = LIP[act] * nu / (1 - nu) * (absaw + bias.double().abs()[:, None]) + U * ref.abs()
    if R is not None:
        rig = rig + U * R.double().abs()[None]
    if act:
        rig = rig + amax(act_fn(act, pre.float()).double() - act_fn(act, pre))
    del absaw
    over = (got - ref).abs() > rig
    print(f"  largest |err| / rigorous fp32 bound of an element: {((got - ref).abs() / rig).max().item():.3e}")
    assert not over.any(), (name, "elements outside the rigorous fp32 bound", torch.nonzero(over)[:5].tolist())
    tanh_gap = amax(gelu_tanh(pre) - F.gelu(pre)) if act == 1 else None
    return route, record("gemm", name, amax(got - ref), bound, sep, tanh_gap)


@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_xg_gemm(gpu_lib, name):
    run_gemm(gpu_lib, name)


def test_xg_gemm_route_table():
    """the predicted route of every case is the one it is written for"""
    got = {name: gemm_route(gemm_case(name)) for name in GEMM_CASES}
    print(got)
    for name, route in got.items():
        assert route == gemm_expected(name), (name, route)


def _gemm_refusal(lib, M, N, K, **kw):
    a = dict(A2=None, lda2=0, a2_mod=1, res=None, ldres=0, res_shift=0, res_mod=0, res_rows_per=0, res_stride=0, res_div=1, res_off=0, act=0,
             act_last=0, pool4=0, a_off=0, lda=K)
    a.update(kw)
    A = torch.randn(a["a_off"] + M * a["lda"] + 8, device="cuda")
    W = torch.randn(N * K, device="cuda")
    C_flat = canary_buf(M * N)
    st = lib.saber_k_xg_gemm(p(A, a["a_off"]), a["lda"], 0, p(a["A2"]), a["lda2"], a["a2_mod"], p(W), K, 0, None, 0, p(a["res"]), a["ldres"], a["res_shift"],
                             a["res_mod"], a["res_rows_per"], a["res_stride"], a["res_div"], a["res_off"], p(C_flat), N, 0, M, N, K, a["act"], a["act_last"],
                             a["pool4"], 1, None)
    torch.cuda.synchronize()
    msg = lib.saber_k_last_error().decode() if st else ""
    assert (C_flat.view(torch.int32) == CANARY).all(), "a refused call wrote its output"
    return st, msg


def test_xg_gemm_refusals(gpu_lib):
    """pool4 with a residual, act_last, A2 or any activation is refused (the kernels would drop the residual / act_last and apply the activation
    after the maximum, unlike launch_gemm), as are pool4 with M % 4 != 0, a shifted / modular residual beyond one row slab of the unaligned
    kernel and the 16-byte rows the fused operand sum needs - before anything is launched"""
    M, N, K = 64, 32, 16
    res = torch.randn(M * N, device="cuda")
    A2 = torch.randn(8 * K, device="cuda")
    pool = "exact gemm: pool4 takes no residual, act_last, A2 or activation"
    for kw in (dict(res=res, ldres=N), dict(act_last=1), dict(A2=A2, lda2=K, a2_mod=8), dict(act=1), dict(act=2), dict(act=3),
               dict(res=res, ldres=N, act_last=1, act=1)):
        st, msg = _gemm_refusal(gpu_lib, M, N, K, pool4=1, **kw)
        print(f"pool4 + {sorted(k for k in kw if k not in ('ldres', 'lda2', 'a2_mod'))}: {msg}")
        assert st == -1 and msg == pool, (kw, msg)
    st, msg = _gemm_refusal(gpu_lib, 62, N, K, pool4=1)
    assert st == -1 and msg == "exact gemm: pool4 needs M % 4 == 0", msg
    st, msg = _gemm_refusal(gpu_lib, M, N, K, A2=A2, lda2=K, a2_mod=8, a_off=1)
    assert st == -1 and msg == "exact gemm: the fused operand sum / slot residual need 16-byte rows", msg
    st, msg = _gemm_refusal(gpu_lib, M, N, 3, res=res, ldres=N, res_rows_per=8, res_stride=8 * N, res_div=1)
    assert st == -1 and msg == "exact gemm: the fused operand sum / slot residual need 16-byte rows", msg
    # a residual row map (shift / modulo) on the unaligned kernel with M beyond one slab of 65 535 row tiles
    Mb, Nb = SLAB_ROWS + 128, 4
    resb = torch.randn(Mb * Nb, device="cuda")
    for kw in (dict(res_shift=1), dict(res_mod=5)):
        st, msg = _gemm_refusal(gpu_lib, Mb, Nb, 3, res=resb, ldres=Nb, **kw)
        assert st == -1 and msg == "exact gemm: residual mapping with M beyond one slab", (kw, msg)
    # the argument checks of the entry point itself
    st, msg = _gemm_refusal(gpu_lib, M, N, K, res=res, ldres=N, res_rows_per=8, res_stride=8 * N, res_div=0)
    assert st == -1 and "res_div" in msg, msg


# ------------------------------------------------------------------------------------------------ attention
# sharp: scores after the scale of order 1e2 (softmax near one-hot), else of order 1.  In every case the top-scoring key is planted at
# j = nk - 1 (in the ragged last key tile where nk % 32 != 0).  kmask: "masked_top" = a key that would score above it is masked, and keys
# 32..63 (a whole 32-key tile) too; "one_live" = every key masked but j = nk - 1.
ATTN_CASES = {}


def _attn(name, route, **kw):
    kw.setdefault("heads", 8 if kw["hd"] == 16 else 2)
    kw.setdefault("batch", 3)
    ATTN_CASES[name] = dict(kw, route=route)


for _s in (0, 1):
    for _nq in (1, 8, 9, 16):       # nk >= 1024, nk % 64 != 0: the last wave's key segment (and its last 16-key block) is ragged
        _attn(f"fewq_mfma_nq{_nq}_sharp{_s}", "attn fewq mfma", hd=16, nq=_nq, nk=4133, batch=24, sharp=_s)
        _attn(f"fewq_valu_nq{_nq}_sharp{_s}", "attn fewq valu", hd=16, nq=_nq, nk=4133 if _s else 1093, batch=24, sharp=_s, ldq=130)
    for _nk in range(1, 17):
        _attn(f"fewk_nk{_nk}_sharp{_s}", "attn fewk", hd=16, nq=300, nk=_nk, batch=3, sharp=_s)
    _attn(f"mfma56_masked_sharp{_s}", "attn mfma<56>", hd=56, nq=300, nk=100, sharp=_s, kmask="masked_top")
    _attn(f"mfma72_qpool_sharp{_s}", "attn mfma<72>", hd=72, nq=77, nk=200, sharp=_s, qpool=1)
    _attn(f"mfma96_sharp{_s}", "attn mfma<96>", hd=96, nq=130, nk=150, heads=1, batch=5, sharp=_s)
    _attn(f"generic16_sharp{_s}", "attn generic<16>", hd=16, nq=300, nk=100, heads=2, sharp=_s)
    _attn(f"generic32_sharp{_s}", "attn generic<32>", hd=32, nq=9, nk=9, heads=8, batch=40, sharp=_s)
    _attn(f"generic56_ldo_sharp{_s}", "attn generic<56>", hd=56, nq=200, nk=70, sharp=_s, ldo=2 * 56 + 1, kmask="masked_top")
    _attn(f"generic72_qpool_sharp{_s}", "attn generic<72>", hd=72, nq=64, nk=256, sharp=_s, qpool=1, o_off=1, kmask="masked_top")
    _attn(f"generic96_ldk_sharp{_s}", "attn generic<96>", hd=96, nq=140, nk=99, heads=1, batch=4, sharp=_s, ldk=97)
_attn("mfma96_one_live", "attn mfma<96>", hd=96, nq=50, nk=150, heads=1, batch=5, sharp=0, kmask="one_live")
_attn("generic72_one_live", "attn generic<72>", hd=72, nq=60, nk=100, sharp=1, kmask="one_live", ldv=2 * 72 + 2)


def attn_layout(a):
    Cq, qrows = a["heads"] * a["hd"], (4 if a.get("qpool") else 1) * a["nq"]
    L = dict(ldq=a.get("ldq", Cq), ldk=a.get("ldk", Cq), ldv=a.get("ldv", Cq), ldo=a.get("ldo", Cq), q_off=a.get("q_off", 0), k_off=0, v_off=0,
             o_off=a.get("o_off", 0), qrows=qrows)
    L.update(q_bs=qrows * L["ldq"], k_bs=a["nk"] * L["ldk"], v_bs=a["nk"] * L["ldv"], o_bs=a["nq"] * L["ldo"])
    return L


def attn_formula(q, k, v, scale, kmask, qpool, dt):
    """ref_hiera_attention's formula: q [B][rows][H][hd] (rows = 4 nq with qpool), k, v [B][nk][H][hd] -> [B][nq][H][hd]"""
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    B, rows, H, hd = q.shape
    if qpool:
        q = q.view(B, rows // 4, 4, H, hd).amax(2)
    q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    sc = torch.matmul(q, k.transpose(-1, -2)) * scale
    if kmask is not None:
        sc = sc.masked_fill(~kmask[None, None, None, :], float("-inf"))
    return torch.matmul(torch.softmax(sc, -1), v).transpose(1, 2), sc


def run_attn(lib, name):
    a = ATTN_CASES[name]
    hd, nq, nk, H, B, qpool = a["hd"], a["nq"], a["nk"], a["heads"], a["batch"], a.get("qpool", 0)
    L = attn_layout(a)
    route = attn_route(a)
    assert route == a["route"], (name, route)
    print(f"\n{name}: hd {hd} nq {nq} nk {nk} heads {H} batch {B} qpool {qpool} kmask {a.get('kmask')} -> {route}")
    gen = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, generator=gen, device="cuda")
    Cq = H * hd
    scale = float(torch.tensor(hd ** -0.5, dtype=torch.float32))
    S, gap = (30.0, 5.0) if a.get("sharp") else (1.0, 2.0)      # spread of the random scores, lead of the planted top key
    e = F.normalize(rn(H, hd), dim=-1)
    q = e[None, None] + 0.3 * rn(B, L["qrows"], H, hd) / math.sqrt(hd)
    if qpool:      # channel d of pooling group i takes its maximum from row (d + i) % 4
        win = (torch.arange(hd, device="cuda")[None, :] + torch.arange(nq, device="cuda")[:, None]) % 4
        bump = F.one_hot(win, 4).permute(0, 2, 1).to(torch.float32)          # [nq][4][hd]
        q = (q.view(B, nq, 4, H, hd) + 1.5 / math.sqrt(hd) * bump[None, :, :, None, :]).view(B, L["qrows"], H, hd)
        frac = (q.view(B, nq, 4, H, hd).argmax(2) == win[None, :, None, :]).float().mean().item()
        assert frac > 0.95, frac
    k = S * math.sqrt(hd) * rn(B, nk, H, hd) / (1.0 + 0.3)
    v = rn(B, nk, H, hd)
    kmask = None
    if a.get("kmask") == "one_live":
        kmask = torch.zeros(nk, dtype=torch.bool, device="cuda")
        kmask[nk - 1] = True
    elif a.get("kmask") == "masked_top":
        kmask = torch.ones(nk, dtype=torch.bool, device="cuda")
        kmask[32:64] = False
        assert nk > 64
    if nk > 1:      # key nk - 1 scores `gap` above the best random key against the mean query of its (batch, head)
        qm = (q.view(B, nq, 4, H, hd).amax(2) if qpool else q).mean(1)       # [B][H][hd]
        live = torch.ones(nk - 1, dtype=torch.bool, device="cuda") if kmask is None else kmask[:nk - 1]
        smax = torch.zeros(B, H, device="cuda")
        if live.any():
            smax = (scale * torch.einsum("bjhd,bhd->bjh", k[:, :nk - 1], qm))[:, live].amax(1)       # [B][H]
        target = torch.clamp(smax + gap, min=3 * S)
        k[:, nk - 1] = qm * (target / scale / qm.pow(2).sum(-1))[..., None]
        if a.get("kmask") == "masked_top":
            jm = nk // 2 + 3
            k[:, jm] = 1.5 * k[:, nk - 1]
            kmask[jm] = False
    # device buffers
    def place(t, rows, ld, bs, off):
        flat = torch.randn(off + (B - 1) * bs + (rows - 1) * ld + Cq + 5, generator=gen, device="cuda")
        strided(flat, (B, rows, Cq), (bs, ld, 1), off).copy_(t.reshape(B, rows, Cq))
        return flat
    qf = place(q, L["qrows"], L["ldq"], L["q_bs"], L["q_off"])
    kf = place(k, nk, L["ldk"], L["k_bs"], 0)
    vf = place(v, nk, L["ldv"], L["v_bs"], 0)
    of = canary_buf(L["o_off"] + (B - 1) * L["o_bs"] + (nq - 1) * L["ldo"] + Cq)
    ov = strided(of, (B, nq, Cq), (L["o_bs"], L["ldo"], 1), L["o_off"])
    km8 = None if kmask is None else kmask.to(torch.uint8)
    kcall(lib, lib.saber_k_xg_attention(hd, p(qf, L["q_off"]), L["q_bs"], L["ldq"], p(kf), L["k_bs"], L["ldk"], p(vf), L["v_bs"], L["ldv"], p(of, L["o_off"]),
                                        L["o_bs"], L["ldo"], nq, nk, B, H, qpool, p(km8), scale, None))
    check_written(of, ov, name)
    got = ov.double().view(B, nq, H, hd)
    ref, sc = attn_formula(q, k, v, scale, kmask, qpool, torch.float64)
    if nk > 1:
        top = (sc.argmax(-1) == nk - 1).double().mean().item()
        live_sc = sc if kmask is None else sc[..., kmask]
        print(f"  scores after the scale: max {amax(live_sc):.1f}, std {live_sc.std().item():.2f}; planted key nk - 1 on top for {100 * top:.0f} % of the queries")
        assert top >= 0.5, "the planted key is not the top-scoring one"
        if a.get("sharp"):
            assert amax(live_sc) >= 50
        else:
            assert amax(live_sc) <= 20
    e_f32 = amax(attn_formula(q, k, v, scale, kmask, qpool, torch.float32)[0].double() - ref)
    sep = amax(attn_formula(q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16), scale, kmask, qpool, torch.float64)[0] - ref)
    return route, record("attention", name, amax(got - ref), 8 * e_f32, sep)


@pytest.mark.parametrize("name", list(ATTN_CASES))
def test_xg_attention(gpu_lib, name):
    run_attn(gpu_lib, name)


def test_xg_attention_refuses_head_dim(gpu_lib):
    t = torch.randn(4 * 10 * 64, device="cuda")
    o = canary_buf(10 * 64)
    st = gpu_lib.saber_k_xg_attention(64, p(t), 640, 64, p(t), 640, 64, p(t), 640, 64, p(o), 640, 64, 10, 10, 1, 1, 0, None, 0.125, None)
    torch.cuda.synchronize()
    assert st == -1 and gpu_lib.saber_k_last_error().decode() == "exact attention: unsupported head dimension"
    assert (o.view(torch.int32) == CANARY).all()


def test_xg_attention_route_table():
    """the predicted route of every case is the one it is written for; every route has a case with scores of order 1 and one of order 1e2"""
    for n, a in ATTN_CASES.items():
        assert attn_route(a) == a["route"], n
    for r in {a["route"] for a in ATTN_CASES.values()}:
        assert {a.get("sharp", 0) for a in ATTN_CASES.values() if a["route"] == r} == {0, 1}, r


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln(name, **kw):
    LN_CASES[name] = kw


LN_CASES = {}
for _C, _rows in ((64, 1001), (256, 1003), (1152, 1001), (1300, 999), (250, 1001)):
    _ln(f"C{_C}", C=_C, rows=_rows)
    _ln(f"C{_C}_bigmean", C=_C, rows=_rows, bigmean=True)
    if _C != 64:
        _ln(f"C{_C}_row_valid", C=_C, rows=_rows, valid_mod=37)
_ln("C64_row_valid", C=64, rows=1001, valid_mod=37)
_ln("C64_gelu", C=64, rows=2001, act=1, eps=1e-6)
_ln("C256_unaligned_gelu", C=256, rows=1003, x_off=1, act=1)


def ln_formula(x, g, b, eps, act, dt, onepass=False):
    x, g, b = x.to(dt), g.to(dt), b.to(dt)
    mu = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mu * mu if onepass else (x - mu).pow(2).mean(-1, keepdim=True)
    pre = (x - mu) / (var + eps).sqrt() * g + b
    return act_fn(act, pre), pre


@pytest.mark.parametrize("name", list(LN_CASES))
def test_xg_layernorm(gpu_lib, name):
    """rows not a multiple of the rows per workgroup, a constant row (fp64 result exactly beta), zero rows of row_valid, and rows whose mean
    is 1e4 times their standard deviation (where a one-pass E[x^2] - mu^2 fails and the two-pass variance does not)"""
    c = LN_CASES[name]
    C_, rows, act, off, vm = c["C"], c["rows"], c.get("act", 0), c.get("x_off", 0), c.get("valid_mod", 0)
    eps = float(torch.tensor(c.get("eps", 1e-5), dtype=torch.float32))
    route = ln_route(c)
    print(f"\n{name}: rows {rows} C {C_} act {act} -> {route}")
    gen = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
    x = torch.randn(rows, C_, generator=gen, device="cuda") * 2 + 0.5
    if c.get("bigmean"):
        x = (1e4 + torch.randn(rows, C_, generator=gen, device="cuda", dtype=torch.float64)).float()
    x[5] = 0.75                                                        # a constant row: x - mean = 0 exactly
    g = 1 + 0.2 * torch.randn(C_, generator=gen, device="cuda")
    b = 0.3 * torch.randn(C_, generator=gen, device="cuda")
    xf = torch.zeros(off + rows * C_, device="cuda")
    xf[off:] = x.reshape(-1)
    rv = None
    if vm:
        rv = (torch.rand(vm, generator=gen, device="cuda") < 0.7).to(torch.uint8)
        rv[5 % vm] = 1
        rv[0] = 0
    out = canary_buf(rows * C_)
    kcall(gpu_lib, gpu_lib.saber_k_xg_layernorm(p(xf, off), p(g), p(b), eps, p(out), rows, C_, act, p(rv), vm, None))
    check_written(out, out[:rows * C_], name)
    got = out[:rows * C_].view(rows, C_).double()
    keep = torch.ones(rows, dtype=torch.bool, device="cuda") if rv is None else rv[torch.arange(rows, device="cuda") % vm].bool()
    ref, pre = ln_formula(x, g, b, eps, act, torch.float64)
    ref[~keep] = 0
    assert torch.equal(got[~keep], ref[~keep]), "row_valid rows must be zeros"
    if act == 0:
        assert torch.equal(ref[5], b.double()) and torch.equal(got[5], b.double()), "a constant row gives exactly beta"
    f32 = ln_formula(x, g, b, eps, act, torch.float32)[0].double()
    f32[~keep] = 0
    e_f32 = amax(f32 - ref)
    if c.get("bigmean"):
        one = ln_formula(x, g, b, eps, act, torch.float32, onepass=True)[0].double()
        e_one = (one - ref)[keep].abs().nan_to_num(math.inf).max().item()
        print(f"  one-pass variance in fp32: {e_one:.3e}, two-pass E_f32 {e_f32:.3e}")
        assert e_f32 * 10 <= e_one
    sep = amax(ln_formula(x.to(torch.bfloat16), g.to(torch.bfloat16), b.to(torch.bfloat16), eps, act, torch.float64)[0][keep] - ref[keep])
    tanh_gap = amax(gelu_tanh(pre) - F.gelu(pre)) if act == 1 else None
    record("layernorm", name, amax(got - ref), 8 * e_f32, sep, tanh_gap)


# ------------------------------------------------------------------------------------------------ elementwise
ADD_CASES = {"C256_ymod7": dict(rows=1001, C=256, ymod=7), "C250_no_mod": dict(rows=1001, C=250, ymod=0)}


@pytest.mark.parametrize("name", list(ADD_CASES))
def test_xg_add(gpu_lib, name):
    c = ADD_CASES[name]
    rows, C_, ymod = c["rows"], c["C"], c["ymod"]
    gen = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
    x = torch.randn(rows, C_, generator=gen, device="cuda")
    y = torch.randn(ymod or rows, C_, generator=gen, device="cuda")
    out = canary_buf(rows * C_)
    kcall(gpu_lib, gpu_lib.saber_k_xg_add(p(x), p(y), ymod, p(out), rows, C_, None))
    check_written(out, out[:rows * C_], name)
    yi = y[torch.arange(rows, device="cuda") % ymod] if ymod else y
    ref = x.double() + yi.double()
    sep = amax(x.to(torch.bfloat16).double() + yi.to(torch.bfloat16).double() - ref)
    record("add", name, amax(out[:rows * C_].view(rows, C_).double() - ref), 8 * amax((x + yi).double() - ref), sep)


ADD_SLOT_CASES = {
    "f4_in_vec": dict(P=6, div=3, off=2, rows_per=100, C=256, stride=100 * 256 + 8, use_in=True, use_vec=True),
    "f4_vec_only_gelu": dict(P=6, div=2, off=1, rows_per=64, C=256, stride=64 * 256 + 4, use_in=False, use_vec=True, act=1),
    "f4_in_only": dict(P=4, div=4, off=3, rows_per=120, C=256, stride=120 * 256, use_in=True, use_vec=False),
    "scalar_C250": dict(P=6, div=3, off=2, rows_per=100, C=250, stride=100 * 250 + 8, use_in=True, use_vec=True),
    "scalar_stride": dict(P=6, div=4, off=1, rows_per=100, C=256, stride=100 * 256 + 3, use_in=True, use_vec=False, act=1),
    "scalar_offset": dict(P=6, div=3, off=2, rows_per=100, C=256, stride=100 * 256 + 8, use_in=False, use_vec=True, off4=1),
}


@pytest.mark.parametrize("name", list(ADD_SLOT_CASES))
def test_xg_add_slot(gpu_lib, name):
    """out[p] = act(in[p] + tab[(p + off) / div] + vec): both forms, the last slot only partly used, vec and in on and off"""
    c = ADD_SLOT_CASES[name]
    P, div, off, rp, C_, stride, act, o4 = c["P"], c["div"], c["off"], c["rows_per"], c["C"], c["stride"], c.get("act", 0), c.get("off4", 0)
    route = add_slot_route(c)
    n_slots = (P - 1 + off) // div + 1
    assert ((P - 1 + off) % div) != div - 1, "the last slot is used by fewer than div prompts"
    print(f"\n{name}: P {P} div {div} off {off} slots {n_slots} -> {route}")
    gen = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
    per = rp * C_
    tab = torch.randn(o4 + n_slots * stride, generator=gen, device="cuda")
    inp = torch.randn(o4 + P * per, generator=gen, device="cuda") if c["use_in"] else None
    vec = torch.randn(o4 + C_, generator=gen, device="cuda") if c["use_vec"] else None
    out = canary_buf(o4 + P * per)
    kcall(gpu_lib, gpu_lib.saber_k_xg_add_slot(p(inp, o4), p(tab, o4), stride, div, off, p(vec, o4), p(out, o4), rp, C_, P, act, None))
    ov = out[o4:o4 + P * per]
    check_written(out, ov, name)
    sl = (torch.arange(P, device="cuda") + off) // div
    T = tab[o4:].as_strided((n_slots, per), (stride, 1))[sl]                     # [P][per]

    def formula(dt, rb=lambda t: t):
        v = rb(T).to(dt)
        if inp is not None:
            v = v + rb(inp[o4:].view(P, per)).to(dt)
        if vec is not None:
            v = v + rb(vec[o4:]).to(dt).repeat(rp)[None]
        return act_fn(act, v), v
    ref, pre = formula(torch.float64)
    sep = amax(formula(torch.float64, lambda t: t.to(torch.bfloat16))[0] - ref)
    tanh_gap = amax(gelu_tanh(pre) - F.gelu(pre)) if act == 1 else None
    record("add_slot", name, amax(ov.view(P, per).double() - ref), 8 * amax(formula(torch.float32)[0].double() - ref), sep, tanh_gap)


# ------------------------------------------------------------------------------------------------ mask prompt: hidden stages and the final product
def mask_weights(gen):
    r = lambda *s: torch.randn(*s, generator=gen, device="cuda")
    return dict(w1=r(4, 1, 2, 2) * 0.5, b1=r(4) * 0.1, g1=1 + 0.1 * r(4), be1=0.1 * r(4), w2=r(16, 4, 2, 2) * 0.3, b2=r(16) * 0.1, g2=1 + 0.1 * r(16),
                be2=0.1 * r(16))


def ln2d(x, g, b):
    mu = x.mean(1, keepdim=True)
    var = (x - mu).pow(2).mean(1, keepdim=True)
    return (x - mu) / (var + 1e-6).sqrt() * g[None, :, None, None] + b[None, :, None, None]


def mask_hidden_formula(m, w, clamp, dt, rb=lambda t: t):
    W = {k: rb(v).to(dt) for k, v in w.items()}
    x = rb(m).to(dt)[:, None]
    if clamp > 0:
        x = x.clamp(-clamp, clamp)
    x = F.gelu(ln2d(F.conv2d(x, W["w1"], W["b1"], stride=2), W["g1"], W["be1"]))
    pre = ln2d(F.conv2d(x, W["w2"], W["b2"], stride=2), W["g2"], W["be2"])
    return F.gelu(pre), pre


@pytest.mark.parametrize("clamp,q0", [(0.0, -1), (20.0, -1), (0.0, 2), (20.0, 5)])
def test_xg_mask_hidden(gpu_lib, clamp, q0):
    """h2 of the mask prompt against two stages of conv2d(k2, s2) + LayerNorm2d + GELU in fp64; clamp_abs on and off (inputs beyond +-20 in
    every plane); raw4_q0 = -1 reads plane p, raw4_q0 >= 0 reads plane i + i / 3 + 1 of i = raw4_q0 + p (every other plane holds garbage that
    would show)"""
    P = 3
    name = f"clamp{clamp:g}_q0{q0}"
    gen = torch.Generator(device="cuda").manual_seed(int(clamp) * 31 + q0 + 7)
    planes = [p_ if q0 < 0 else (q0 + p_) + (q0 + p_) // 3 + 1 for p_ in range(P)]
    mask_in = torch.randn(max(planes) + 2, 256, 256, generator=gen, device="cuda") * 12
    w = mask_weights(gen)
    out = canary_buf(P * 4096 * 16)
    kcall(gpu_lib, gpu_lib.saber_k_xg_mask_hidden(p(mask_in), P, *(p(w[k]) for k in ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2")), clamp, q0,
                                                  p(out), None))
    check_written(out, out[:P * 4096 * 16], name)
    m = mask_in[planes]
    if clamp > 0:
        assert (m.abs() > clamp).float().mean().item() > 0.05
    idx = perm_grid(gpu_lib, 2, "cuda")
    ref, pre = mask_hidden_formula(m, w, clamp, torch.float64)
    got = out[:P * 4096 * 16].view(P, 4096, 16).double()
    ref_e = to_engine_order(ref, idx)
    e_f32 = amax(to_engine_order(mask_hidden_formula(m, w, clamp, torch.float32)[0].double(), idx) - ref_e)
    sep = amax(to_engine_order(mask_hidden_formula(m, w, clamp, torch.float64, lambda t: t.to(torch.bfloat16))[0], idx) - ref_e)
    record("mask_hidden", name, amax(got - ref_e), 8 * e_f32, sep, amax(gelu_tanh(pre) - F.gelu(pre)))


@pytest.mark.parametrize("P", [1, 3])
def test_xg_mask_dot(gpu_lib, P):
    """masks4[p][k][y][x] = sum_c hyper[p][k][c] up[p][perm(y, x)][c] (an einsum in fp64), token order from saber_k_perm_index"""
    gen = torch.Generator(device="cuda").manual_seed(P)
    up = torch.randn(P, 65536, 32, generator=gen, device="cuda")
    hyper = torch.randn(P, 4, 32, generator=gen, device="cuda")
    out = canary_buf(P * 4 * 65536)
    kcall(gpu_lib, gpu_lib.saber_k_xg_mask_dot(p(up), p(hyper), P, p(out), None))
    check_written(out, out[:P * 4 * 65536], f"mask_dot P {P}")
    idx = perm_grid(gpu_lib, 0, "cuda")
    f = lambda u, h, dt: torch.einsum("pkc,ptc->pkt", h.to(dt), u.to(dt))[:, :, idx]
    ref = f(up, hyper, torch.float64)
    sep = amax(f(up.to(torch.bfloat16), hyper.to(torch.bfloat16), torch.float64) - ref)
    record("mask_dot", f"P {P}", amax(out[:P * 4 * 65536].view(P, 4, 65536).double() - ref), 8 * amax(f(up, hyper, torch.float32).double() - ref), sep)


# ------------------------------------------------------------------------------------------------ coverage
def test_every_route_has_a_case():
    """the case tables reach every route of the dispatchers (ROUTES): a route added to exact.hip and to ROUTES without a case fails here"""
    assert torch.cuda.is_available()
    have = {gemm_route(gemm_case(n)) for n in GEMM_CASES} | {attn_route(a) for a in ATTN_CASES.values()} | {ln_route(c) for c in LN_CASES.values()}
    have |= {add_slot_route(c) for c in ADD_SLOT_CASES.values()} | {"add", "mask_hidden", "mask_dot"}
    missing = set(ROUTES) - have
    unknown = have - set(ROUTES)
    assert not missing and not unknown, (sorted(missing), sorted(unknown))
    assert len(ROUTES) == len(set(ROUTES))
