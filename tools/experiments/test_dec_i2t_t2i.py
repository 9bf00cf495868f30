"""Parity test of the parked experiment tools/experiments/dec_i2t_t2i.hip (not collected by the suites: the kernel is not in the library).
To run it: revive the kernel as tools/experiments/README.md says, copy this file to tests/ (was tests/test_gpu_fused_i2t_t2i.py).

The fused kernel `dec_i2t_t2i_kernel` (image -> tokens of a decoder layer + the tokens -> image attention that follows it,
SABER_AMD_FUSE_I2T_T2I=1) against the two separate launches it replaces (sam2 two_way_transformer: TwoWayAttentionBlock.forward's
cross_attn_image_to_token followed by the next block's / the final cross_attn_token_to_image).

X' (the updated image tokens) is computed by the same instructions in both forms and must be bit-identical - visible in the mask logits of
prompts whose tokens did not change; the attention over X' differs only in the grouping of the online softmax (32-key blocks in one wave
instead of 64-key blocks in two), so the decode's outputs agree to the operand format's rounding."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_fused_equals_separate_launches(precision):
    from saber_amd.engine import Engine
    eng = Engine("large", device=0, seed=0, max_images=1, max_prompts=1024, precision=precision)
    try:
        g = torch.Generator(device="cpu").manual_seed(3)
        eng.encode(torch.rand(1024, 1024, generator=g).cuda())
        pts = (torch.rand(1024, 2, generator=g) * 1024).cuda()
        outs = {}
        for fuse in (False, True):
            if fuse:
                os.environ["SABER_AMD_FUSE_I2T_T2I"] = "1"
            else:
                os.environ.pop("SABER_AMD_FUSE_I2T_T2I", None)
            low, iou, _ = eng.decode_points(pts, slot=0, multimask=True)
            mi = torch.clamp(low[:, 0], -32, 32).contiguous()
            low2, iou2, _ = eng.decode_points(pts, slot=0, multimask=False, mask_input=mi)
            torch.cuda.synchronize()
            outs[fuse] = [t.float().cpu().numpy() for t in (low, iou, low2, iou2)]
        eng.check_finite()
        tol = {"bf16": 2e-2, "fp16": 3e-3}[precision]
        for name, a, b in zip(("logits", "pred_iou", "m2m logits", "m2m pred_iou"), outs[False], outs[True]):
            scale = max(1.0, float(np.abs(a).max()))
            err = float(np.abs(a - b).max()) / scale
            print(f"{precision} fused vs separate, {name}: max |diff| / max|ref| = {err:.2e} (scale {scale:.1f})")
            assert np.isfinite(b).all()
            assert err < tol, name
            if "logits" in name:
                assert ((a > 0) != (b > 0)).mean() < 2e-3
    finally:
        os.environ.pop("SABER_AMD_FUSE_I2T_T2I", None)
        eng.close()
