"""GPU: the fused MLP row-owner kernel (csrc/gemm_mlp_rowln.hip: mlp.layers.0 + GELU + mlp.layers.1 + residual + the next LayerNorm, the
hidden activation stays on chip) against the pair of launches it replaces in the stage-0 blocks of Hiera-L - saber_k_gemm_ld (GELU, 16-bit
out) followed by saber_k_gemm_rowln - through the kernel-level C-ABI, and inside the engine through development flag 262144 (which restores
the pair).

The kernel keeps the pair's rounding model (fp32 accumulation with 16x16x32 MFMAs over ascending K from a zero accumulator, bias in fp32, the
same GELU on the same value pairs, h rounded to the operand type, the shared epilogue), so the target is bit-equality of every output.
IT HOLDS: y, the 16-bit copy and the LayerNorm rows are bit-equal to the pair's for both operand types at every shape below; the errors of
both paths against an fp64 evaluation on the same 16-bit operands (h rounded to the type) are printed and, being those of the same bits, equal
(measured at M = 76 817: max-abs / max|y| 2.9e-4 bf16, 4.6e-5 fp16; relative RMS 8.1e-5 / 2.9e-5; LayerNorm rows <= 1 ulp of the type).

Shapes: T = 256 rows per tile.  2 T + 37: a ragged last tile; 300 T + 17: more tiles than workgroups (uneven persistent walks).  One set of
inputs per operand type: the small problem is the head of the large one (row independence), the pair runs once per problem."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.op16 import DTYPE, OPS, operand_type, rnd
from tests.test_gpu_kernels import amax, kcall, ptr

pytestmark = pytest.mark.gpu

CW, T = 144, 256
M_SMALL, M_BIG = 2 * T + 37, 300 * T + 17
NO_MLPFUSE = 262144          # development flag: the engine runs the pair of launches


@functools.lru_cache(maxsize=None)
def inputs(op):
    """xn, the padded weights the engine uploads (rows zero-padded to a multiple of 64 in K), biases, residual, LayerNorm parameters"""
    g = torch.Generator(device="cuda").manual_seed(144 + (op == "fp16"))
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    A = (r(M_BIG, CW) * 0.9).to(DTYPE[op])
    W1 = torch.zeros(4 * CW, 192, dtype=DTYPE[op], device="cuda")
    W1[:, :CW] = (r(4 * CW, CW) / CW ** 0.5).to(DTYPE[op])
    W2 = (r(CW, 4 * CW) / (4 * CW) ** 0.5).to(DTYPE[op])
    b1, b2 = r(4 * CW) * 0.5, r(CW)
    res = r(M_BIG, CW) * 2 + 0.5
    gamma, beta = torch.rand(CW, device="cuda", generator=g) + 0.5, r(CW) * 0.1
    return A, W1, W2, b1, b2, res, gamma, beta


def run_fused(lib, op, M, with_bf=True, alias_ln=False):
    A, W1, W2, b1, b2, res, gamma, beta = inputs(op)
    y = res[:M].clone()                                      # in place: res aliases out_f32, as the engine's residual stream does
    yb = torch.zeros(M, CW, dtype=DTYPE[op], device="cuda") if with_bf else None
    a = A[:M].clone() if alias_ln else A                     # alias_ln: the LayerNorm rows overwrite xn, as e->xn does in the engine
    ln = a if alias_ln else torch.zeros(M, CW, dtype=DTYPE[op], device="cuda")
    with operand_type(lib, op):
        kcall(lib, lib.saber_k_mlp_rowln(ptr(a), CW, ptr(W1), 192, ptr(b1), ptr(W2), 4 * CW, ptr(b2), ptr(y), ptr(y), ptr(yb), ptr(gamma), ptr(beta), 1e-6,
                                         ptr(ln), M, CW, None))
    return y, yb, ln


@functools.lru_cache(maxsize=None)
def pair(lib, op, M):
    """the parent's two launches on the same inputs: (y, 16-bit copy of y, LayerNorm rows, h)"""
    A, W1, W2, b1, b2, res, gamma, beta = inputs(op)
    h = torch.zeros(M, 4 * CW, dtype=DTYPE[op], device="cuda")
    y = res[:M].clone()
    yb = torch.zeros(M, CW, dtype=DTYPE[op], device="cuda")
    ln = torch.zeros(M, CW, dtype=DTYPE[op], device="cuda")
    with operand_type(lib, op):
        kcall(lib, lib.saber_k_gemm_ld(ptr(A), CW, ptr(W1), 192, 1, ptr(b1), None, None, ptr(h), M, 4 * CW, CW, 1, None))
        kcall(lib, lib.saber_k_gemm_rowln(ptr(h), 4 * CW, ptr(W2), 4 * CW, ptr(b2), ptr(y), ptr(y), ptr(yb), ptr(gamma), ptr(beta), 1e-6, ptr(ln), M, CW, 4 * CW, None))
    return y, yb, ln, h


@functools.lru_cache(maxsize=None)
def ref64(op, M):
    """fp64 on the same 16-bit operands, h rounded to the type (exact-erf GELU: the kernels' fitted form is within 2.6e-5 of it, both paths alike)"""
    A, W1, W2, b1, b2, res, gamma, beta = inputs(op)
    h = F.gelu(A[:M].double() @ W1[:, :CW].double().T + b1.double()).to(DTYPE[op])
    return h.double() @ W2.double().T + b2.double() + res[:M].double()


def errors(y, ref):
    d = y.double() - ref
    return amax(d) / amax(ref), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@pytest.mark.parametrize("M,with_bf", [(M_SMALL, True), (M_SMALL, False), (M_BIG, True)])
@pytest.mark.parametrize("op", OPS)
def test_mlp_rowln_matches_the_pair(gpu_lib, op, M, with_bf):
    y, yb, ln = run_fused(gpu_lib, op, M, with_bf)
    py, pyb, pln, _ = pair(gpu_lib, op, M)
    ref = ref64(op, M)
    (fm, fr), (pm, pr) = errors(y, ref), errors(py, ref)
    print(f"mlp_rowln [{op}] M={M}: against fp64 max-abs / max|y| fused {fm:.3e} pair {pm:.3e}; relative RMS fused {fr:.3e} pair {pr:.3e}; "
          f"y differs from the pair's in {(y != py).sum().item()} of {y.numel()} values, the LayerNorm rows in {(ln != pln).sum().item()}")
    assert torch.equal(y, py)                                 # the target of the rounding model: the pair's bits
    assert torch.equal(ln, pln)
    assert fm <= 1.5 * pm and fr <= 1.5 * pr                  # (implied by the above; the yardstick were the bits ever to part)
    if with_bf:
        assert torch.equal(yb.float(), rnd(y, op)) and torch.equal(yb, pyb)
    _, _, _, _, _, _, gamma, beta = inputs(op)
    ln_self = F.layer_norm(y, (CW,), gamma, beta, 1e-6)
    d = (ln.float() - rnd(ln_self, op)).abs()
    ulp = ln_self.abs().clamp(min=1e-3) * (2.0 ** -7 if op == "bf16" else 2.0 ** -10)      # one ulp of the type (an upper bound)
    print(f"mlp_rowln [{op}] LayerNorm rows against LayerNorm of the kernel's own y: max |d| / ulp {float((d / ulp).max()):.3f} (bound 1)")
    assert (d <= ulp).all()
    assert (d > 0).float().mean().item() < 2e-3               # rounding flips only


@pytest.mark.parametrize("op", OPS)
def test_mlp_rowln_rows_do_not_depend_on_the_problem(gpu_lib, op):
    """the first 2 T + 37 rows computed alone and as the head of the 300 T + 17 problem (other tiles, other workgroups, a full tile where the
    small problem has its ragged one): the same bits; and with the LayerNorm rows written over xn, as the engine does"""
    ys, ybs, lns = run_fused(gpu_lib, op, M_SMALL)
    yl, ybl, lnl = run_fused(gpu_lib, op, M_BIG)
    assert torch.equal(ys, yl[:M_SMALL]) and torch.equal(lns, lnl[:M_SMALL]) and torch.equal(ybs, ybl[:M_SMALL])
    ya, yba, lna = run_fused(gpu_lib, op, M_BIG, alias_ln=True)
    assert torch.equal(ya, yl) and torch.equal(lna, lnl) and torch.equal(yba, ybl)


@pytest.mark.parametrize("op", OPS)
def test_mlp_rowln_is_run_to_run_identical(gpu_lib, op):
    outs = [run_fused(gpu_lib, op, M_BIG) for _ in range(4)]
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o))


@pytest.mark.parametrize("op", OPS)
def test_engine_features_with_and_without_the_fused_mlp(gpu_lib, large_weights, image, op):
    """one Hiera-L handle, one slice: features with the pair (flag) and with the fused launch are equal, the fused launch really replaces two
    launches per stage-0 block, and a crop encoded alone and as one of three gives the same bits"""
    from saber_amd.engine import Engine
    _, W = large_weights
    eng = Engine("large", device=0, weights=W, max_images=3, max_prompts=8, precision=op)
    img = torch.from_numpy(image).cuda()
    crops = [[0, 0, 1024, 1024], [128, 64, 768, 704], [300, 200, 1024, 900]]
    try:
        feats, launches = {}, {}
        for mode, flag in (("pair", NO_MLPFUSE), ("fused", 0)):
            gpu_lib.saber_k_set_debug(flag)
            try:
                eng.profile_begin()
                eng.encode(img, crops)
                torch.cuda.synchronize()
                launches[mode] = eng.profile_end()["gemm_bf16"]["launches"]
            finally:
                gpu_lib.saber_k_set_debug(0)
            feats[mode] = [{k: v.clone() for k, v in eng.get_features(s).items()} for s in range(3)]
        assert launches["pair"] - launches["fused"] == 2, launches          # blocks 0 and 1: two launches become one
        for s in range(3):
            for k in ("image_embed", "feat_s0", "feat_s1"):
                assert torch.equal(feats["pair"][s][k], feats["fused"][s][k]), (s, k)
        eng.encode(img, [crops[1]])
        alone = eng.get_features(0)
        for k in ("image_embed", "feat_s0", "feat_s1"):
            assert torch.equal(alone[k], feats["fused"][1][k]), k
    finally:
        eng.close()
