"""GPU: the kernel-level entry points that no other test calls directly (include/saber_amd_kernels.h), each against a plain
fp64 / numpy / scipy restatement; the ones with 16-bit operands or outputs in both operand types (tests/op16.py)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.op16 import DTYPE, OPS, check_bound, operand_type, rnd

pytestmark = pytest.mark.gpu


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def kcall(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()
    torch.cuda.synchronize()


@pytest.mark.parametrize("op", OPS)
def test_gemm_batched_explicit_strides(gpu_lib, op):
    """C[b] = A[b] W[b]^T + bias with padded leading dimensions and batch strides larger than a batch entry: each entry against fp64, the
    padding between rows and entries untouched"""
    M, N, K, B = 300, 136, 192, 3
    lda, ldw, ldcf, ldcb = K + 8, K + 16, N + 4, N + 8
    sA, sW, sCf, sCb = M * lda + 64, N * ldw + 24, M * ldcf + 32, M * ldcb + 16
    g = torch.Generator(device="cuda").manual_seed(41)
    A = torch.randn(B * sA, device="cuda", generator=g).to(DTYPE[op])
    W = (torch.randn(B * sW, device="cuda", generator=g) / K ** 0.5).to(DTYPE[op])
    bias = torch.randn(N, device="cuda", generator=g)
    of = torch.full((B * sCf,), 7.0, device="cuda")
    ob = torch.full((B * sCb,), 7.0, device="cuda", dtype=DTYPE[op])
    with operand_type(gpu_lib, op):
        kcall(gpu_lib, gpu_lib.saber_k_gemm_batched(ptr(A), lda, sA, ptr(W), ldw, sW, ptr(bias), ptr(of), ldcf, sCf, ptr(ob), ldcb, sCb, M, N, K, B, None))
    touched_f = torch.zeros(B * sCf, dtype=torch.bool, device="cuda")
    touched_b = torch.zeros(B * sCb, dtype=torch.bool, device="cuda")
    for b in range(B):
        a = A[b * sA: b * sA + M * lda].view(M, lda)[:, :K].double()
        w = W[b * sW: b * sW + N * ldw].view(N, ldw)[:, :K].double()
        ref = a @ w.T + bias.double()
        gf = of[b * sCf: b * sCf + M * ldcf].view(M, ldcf)[:, :N].double()
        gb = ob[b * sCb: b * sCb + M * ldcb].view(M, ldcb)[:, :N].double()
        touched_f[b * sCf: b * sCf + M * ldcf].view(M, ldcf)[:, :N] = True
        touched_b[b * sCb: b * sCb + M * ldcb].view(M, ldcb)[:, :N] = True
        scale = ref.abs().max().item()
        sep = (rnd(ref, "bf16").double() - ref).abs().max().item() / scale
        check_bound(op, f"batch entry {b}: fp32 out", (gf - ref).abs().max().item() / scale, 2e-5)
        check_bound(op, f"batch entry {b}: 16-bit out", (gb - ref).abs().max().item() / scale, 5e-3, 5e-3 / 8, sep)
    assert (of[~touched_f] == 7.0).all() and (ob[~touched_b].float() == 7.0).all(), "a write outside the batch entries' rows"


@pytest.mark.parametrize("op", OPS)
def test_add_to_bf16(gpu_lib, op):
    """out = x + y[row % y_rows] in fp32, rounded once to the operand type: each output alone and both together, y broadcast over rows
    and y NULL - bit-exact (one fp32 add, one RNE)"""
    rows, Cc, y_rows = 1000, 256, 7
    g = torch.Generator(device="cuda").manual_seed(43)
    x = torch.randn(rows, Cc, device="cuda", generator=g) * 300
    y = torch.randn(y_rows, Cc, device="cuda", generator=g) * 300
    ref = x + y.repeat((rows + y_rows - 1) // y_rows, 1)[:rows]
    for yy, r in ((y, ref), (None, x)):
        for want16, want32 in ((True, False), (False, True), (True, True)):
            o16 = torch.zeros(rows, Cc, device="cuda", dtype=DTYPE[op]) if want16 else None
            o32 = torch.zeros(rows, Cc, device="cuda") if want32 else None
            with operand_type(gpu_lib, op):
                kcall(gpu_lib, gpu_lib.saber_k_add_to_bf16(ptr(x), ptr(yy), y_rows, ptr(o16), ptr(o32), rows, Cc, None))
            if want16:
                assert torch.equal(o16.float(), rnd(r, op)), (op, yy is None, want32)
            if want32:
                assert torch.equal(o32, r), (op, yy is None, want16)


@pytest.mark.parametrize("op", OPS)
def test_bf16_to_f32_every_bit_pattern(gpu_lib, op):
    """all 65 536 16-bit patterns widened to fp32 under the operand type: exact (fp16 subnormals included, infinities and signed zeros
    kept), NaN stays NaN"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.uint16)
    ref = bits.view(DTYPE[op]).float()
    x = bits.cuda()
    out = torch.full((65536,), 123.0, device="cuda")
    with operand_type(gpu_lib, op):
        kcall(gpu_lib, gpu_lib.saber_k_bf16_to_f32(ptr(x), 65536, ptr(out), None))
    got = out.cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan].view(torch.int32), ref[~nan].view(torch.int32))
    print(f"{op}: {int(nan.sum())} NaN patterns, {int((~nan).sum())} exact")


def test_axpy_with_and_without_x_and_g(gpu_lib):
    """out = x + alpha g[c] y, x and / or g NULL: against fp64 within the rounding of the fp32 evaluation"""
    rows, Cc, alpha = 3001, 192, -0.375
    g_ = torch.Generator(device="cuda").manual_seed(47)
    x = torch.randn(rows, Cc, device="cuda", generator=g_)
    y = torch.randn(rows, Cc, device="cuda", generator=g_) * 5
    gg = torch.randn(Cc, device="cuda", generator=g_)
    for xx in (x, None):
        for gv in (gg, None):
            out = torch.full((rows, Cc), float("nan"), device="cuda")
            kcall(gpu_lib, gpu_lib.saber_k_axpy(ptr(xx), ptr(y), ptr(gv), alpha, rows, Cc, ptr(out), None))
            t = alpha * y.double() * (gv.double() if gv is not None else 1.0)
            ref = t + (xx.double() if xx is not None else 0.0)
            tol = 2.0 ** -22 * (t.abs() + (xx.double().abs() if xx is not None else 0.0)) + 1e-30
            e = ((out.double() - ref).abs() / tol).max().item()
            print(f"axpy x {'given' if xx is not None else 'NULL'}, g {'given' if gv is not None else 'NULL'}: max err {e:.3f} fp32 roundings")
            assert e <= 1.0


def test_transposed_convolutions_equal_their_twins(gpu_lib):
    """conv3x3s2_t ((3,3,Cin,Cout) weights) and dwconv7_t ((7,7,C) weights): bit-equal to conv3x3s2 / dwconv7 on the same weights, and
    against F.conv2d in fp64"""
    g = torch.Generator().manual_seed(53)
    for (H, Cin, Cout) in ((64, 1, 4), (32, 4, 16), (16, 64, 256), (30, 3, 8)):
        x = torch.randn(1, Cin, H, H, generator=g)
        w, b = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.3, torch.randn(Cout, generator=g)
        ref = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)[0].permute(1, 2, 0).reshape(-1, Cout)
        xd, wd, wtd, bd = x[0].permute(1, 2, 0).contiguous().cuda(), w.cuda(), w.permute(2, 3, 1, 0).contiguous().cuda(), b.cuda()
        Ho = (H + 1) // 2
        o, ot = torch.empty(Ho * Ho, Cout, device="cuda"), torch.empty(Ho * Ho, Cout, device="cuda")
        kcall(gpu_lib, gpu_lib.saber_k_conv3x3s2(ptr(xd), H, H, Cin, ptr(wd), ptr(bd), Cout, ptr(o), None))
        kcall(gpu_lib, gpu_lib.saber_k_conv3x3s2_t(ptr(xd), H, H, Cin, ptr(wtd), ptr(bd), Cout, ptr(ot), None))
        e = (ot.cpu().double() - ref).abs().max().item() / (1 + ref.abs().max().item())
        print(f"conv3x3s2_t {H}x{H}x{Cin}->{Cout}: vs fp64 {e:.2e}, bit-equal to conv3x3s2: {torch.equal(o, ot)}")
        assert torch.equal(o, ot) and e < 1e-5
    for (H, Cc) in ((64, 256), (17, 12)):
        x = torch.randn(1, Cc, H, H, generator=g)
        w, b = torch.randn(Cc, 1, 7, 7, generator=g) * 0.2, torch.randn(Cc, generator=g)
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=3, groups=Cc)[0].permute(1, 2, 0).reshape(-1, Cc)
        xd, wd, wtd, bd = x[0].permute(1, 2, 0).contiguous().cuda(), w.cuda(), w[:, 0].permute(1, 2, 0).contiguous().cuda(), b.cuda()
        o, ot = torch.empty(H * H, Cc, device="cuda"), torch.empty(H * H, Cc, device="cuda")
        kcall(gpu_lib, gpu_lib.saber_k_dwconv7(ptr(xd), H, H, Cc, ptr(wd), ptr(bd), ptr(o), None))
        kcall(gpu_lib, gpu_lib.saber_k_dwconv7_t(ptr(xd), H, H, Cc, ptr(wtd), ptr(bd), ptr(ot), None))
        e = (ot.cpu().double() - ref).abs().max().item() / (1 + ref.abs().max().item())
        print(f"dwconv7_t {H}x{H}x{Cc}: vs fp64 {e:.2e}, bit-equal to dwconv7: {torch.equal(o, ot)}")
        assert torch.equal(o, ot) and e < 1e-5


def test_paint_nearest(gpu_lib):
    """plane[y][x] = label where the logit at the nearest source pixel of the output pixel centre is > thr, other pixels untouched; any_flag
    OR-ed with 1 when a pixel was painted and left alone when none was"""
    g = torch.Generator().manual_seed(59)
    for (Hv, Wv, H, W) in ((256, 256, 1024, 1024), (256, 256, 300, 170), (64, 48, 1000, 37)):
        lg = torch.randn(Hv, Wv, generator=g) * 3
        plane0 = torch.randint(0, 5, (H, W), generator=g, dtype=torch.int32).to(torch.uint16)
        ys = np.clip(np.floor((np.arange(H) + 0.5) * Hv / H).astype(int), 0, Hv - 1)
        xs = np.clip(np.floor((np.arange(W) + 0.5) * Wv / W).astype(int), 0, Wv - 1)
        hit = lg.numpy()[ys[:, None], xs[None, :]] > 0.5
        ref = plane0.numpy().copy()
        ref[hit] = 4321
        plane = plane0.cuda()
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        ld = lg.cuda()
        kcall(gpu_lib, gpu_lib.saber_k_paint_nearest(ptr(ld), Hv, Wv, 0.5, 4321, ptr(plane), H, W, ptr(flag), None))
        assert np.array_equal(plane.cpu().numpy(), ref) and int(flag.item()) == 1, (Hv, Wv, H, W)
    flag = torch.full((1,), 2, dtype=torch.int32, device="cuda")
    ld = torch.full((16, 16), -1.0, device="cuda")
    plane = torch.full((64, 64), 9, dtype=torch.uint16, device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_paint_nearest(ptr(ld), 16, 16, 0.0, 3, ptr(plane), 64, 64, ptr(flag), None))
    assert int(flag.item()) == 2 and (plane.cpu() == 9).all()              # nothing above the threshold: plane and flag untouched
    kcall(gpu_lib, gpu_lib.saber_k_paint_nearest(ptr(ld), 16, 16, -2.0, 3, ptr(plane), 64, 64, None, None))
    assert (plane.cpu() == 3).all()                                         # no flag pointer


def test_gauss_mirror_against_scipy(gpu_lib):
    """one axis of scipy.ndimage.gaussian_filter1d(mode="mirror", truncate=4) on a stack of planes, both axes, sigmas from a one-pixel
    radius to one of 29 pixels on a 40-pixel axis"""
    from scipy import ndimage as ndi
    rng = np.random.default_rng(61)
    for (n, H, W) in ((2, 300, 170), (1, 40, 1100)):
        x = rng.normal(0, 1, (n, H, W)).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        for axis in (0, 1):
            for sigma in (0.25, 1.5, 7.3):
                out = torch.empty_like(xd)
                kcall(gpu_lib, gpu_lib.saber_k_gauss_mirror(ptr(xd), ptr(out), n, H, W, axis, sigma, None))
                ref = ndi.gaussian_filter1d(x.astype(np.float64), sigma, axis=1 + axis, mode="mirror", truncate=4.0)
                e = np.abs(out.cpu().numpy() - ref).max()
                print(f"gauss_mirror {n}x{H}x{W} axis {axis} sigma {sigma}: max abs diff {e:.2e}")
                assert e < 2e-6, (n, H, W, axis, sigma)
