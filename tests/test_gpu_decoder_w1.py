"""GPU: the one-wave-per-SIMD image-side decoder kernels `dec_t2i_w1_kernel` and `dec_i2t_w1_kernel` (csrc/decoder_fused.hip; the default routes
of the tokens -> image attention over a whole key range and of the image -> tokens attention with P >= 512 prompts; SABER_AMD_T2I_W1=0 /
SABER_AMD_I2T_W1=0 and the debug flags select the earlier 8-wave / four-wave kernels): each against fp64 and against the kernel it replaced
on the same operands, in both operand-type builds, and a whole decode on the default route against the 8-wave route."""
import os

import numpy as np
import pytest
import torch

from tests.op16 import check_bound, params

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize(*params("shared", [False, True]))
def test_t2i_one_wave_per_simd_kernel_against_fp64(op, shared):
    """`dec_t2i_w1_kernel` (the route for whole-key-range launches; debug flag 0x20000000 / SABER_AMD_T2I_W1=0 select the 8-wave kernel): the tokens -> image attention with a wave per key quarter and all
    four query tiles per wave - against the same fp64 restatement tests/test_gpu_kernels.py::test_dec_t2i uses, and run-to-run identical
    (it orders its LDS-DMA ring by counted waits alone).  Both operand-type builds."""
    from saber_amd import _lib
    from tests.test_gpu_kernels import check_t2i, t2i_inputs, t2i_launch, t2i_ref
    lib = _lib.load()
    assert lib.saber_k_init(0) == 0
    d = t2i_inputs(300, shared, 11, op)
    lib.saber_k_set_debug(0x10000000)
    try:
        outs = [t2i_launch(lib, d) for _ in range(3)]
    finally:
        lib.saber_k_set_debug(0)
    lib.saber_k_set_debug(0x20000000)
    try:
        ref8 = t2i_launch(lib, d)
    finally:
        lib.saber_k_set_debug(0)
    ref = t2i_ref(d)
    print(f"dec_t2i_w1 (shared={shared}, {op}): the 8-wave kernel's max err {(ref8.double() - ref).abs().max().item():.3e} of scale {ref.abs().max().item():.3f}")
    check_t2i(op, "dec_t2i_w1", outs[0].double(), ref)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_decode_with_t2i_w1_equals_default():
    from saber_amd.engine import Engine
    eng = Engine("large", device=0, seed=0, max_images=1, max_prompts=1024, precision="fp16")
    try:
        g = torch.Generator(device="cpu").manual_seed(4)
        eng.encode(torch.rand(1024, 1024, generator=g).cuda())
        pts = (torch.rand(1024, 2, generator=g) * 1024).cuda()
        outs = {}
        for w1 in (False, True):
            if w1:
                os.environ.pop("SABER_AMD_T2I_W1", None)       # the default route
            else:
                os.environ["SABER_AMD_T2I_W1"] = "0"
            low, iou, _ = eng.decode_points(pts, slot=0, multimask=True)
            mi = torch.clamp(low[:, 0], -32, 32).contiguous()
            low2, iou2, _ = eng.decode_points(pts, slot=0, multimask=False, mask_input=mi)
            torch.cuda.synchronize()
            outs[w1] = [t.float().cpu().numpy() for t in (low, iou, low2, iou2)]
        eng.check_finite()
        for name, a, b in zip(("logits", "pred_iou", "m2m logits", "m2m pred_iou"), outs[False], outs[True]):
            scale = max(1.0, float(np.abs(a).max()))
            err = float(np.abs(a - b).max()) / scale
            print(f"fp16, t2i one-wave-per-SIMD vs default, {name}: max |diff| / max|ref| = {err:.2e}")
            assert np.isfinite(b).all() and err < 3e-3, name
    finally:
        os.environ.pop("SABER_AMD_T2I_W1", None)
        eng.close()


@pytest.mark.parametrize(*params("shared", [False, True]))
def test_i2t_one_wave_per_simd_kernel(op, shared):
    """`dec_i2t_w1_kernel` (the route for whole-prompt launches: P >= 512; debug flag 0x40000000 / SABER_AMD_I2T_W1=0 select the four-wave
    kernel): a wave owns a 16-row tile - all 64 score columns, all 256 channels, softmax weights and LayerNorm statistics in registers.
    Against the fp64 formula of tests/test_gpu_kernels.py::test_dec_i2t on the first prompts, against the four-wave kernel on all of
    them (same operands, same roundings: one 16-bit ulp at most apart), in place (X = Xout: layer 1 of the decoder), run-to-run identical.
    Both operand-type builds."""
    from saber_amd import _lib
    from tests.test_gpu_kernels import check_i2t, i2t_inputs, i2t_launch, i2t_ref, sep_maxabs
    lib = _lib.load()
    assert lib.saber_k_init(0) == 0
    d = i2t_inputs(520, shared, 23, op)

    def run(flag, inplace=False):
        lib.saber_k_set_debug(flag)
        try:
            if inplace:
                out = d["X"].clone()
                return i2t_launch(lib, d, X=out, out=out)
            return i2t_launch(lib, d)
        finally:
            lib.saber_k_set_debug(0)

    w1 = run(0)
    ref4 = run(0x40000000)
    assert torch.equal(w1, run(0)), "run-to-run"
    dd = (w1.float() - ref4.float()).abs()
    print(f"dec_i2t_w1 vs the four-wave kernel (shared={shared}, {op}): differing elements {(dd > 0).float().mean().item():.2e}")
    # one 16-bit ulp of the O(4) outputs at most (0.04 = 1.3 bf16 ulps at 4..8); the fp16 bound must stay below one bf16 rounding of w1
    check_bound(op, "dec_i2t_w1 vs the four-wave kernel, max |diff|", dd.max().item(), 0.04 + 1e-9, 0.04 / 8, sep_maxabs(w1.double()))
    assert (dd > 0).float().mean().item() < 0.05
    if not shared:
        assert torch.equal(w1, run(0, inplace=True)), "in place"
    check_i2t(op, "dec_i2t_w1 vs fp64", w1[:3].double(), i2t_ref(d, 3))
