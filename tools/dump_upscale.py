"""sha256 of dec_upscale_kernel's masks4 for one fixed seeded input (development: bit-identity of two builds of the library).

    python tools/dump_upscale.py [DIR]        (on the GPU box; SABER_AMD_LIB=<path> picks another build of the library)

P = 64 prompts, 8 per crop slot, through saber_k_dec_upscale with iou4 given: a multimask decode (planes 1-3) and a single-mask decode
(plane 0 + the best of 1-3), with bf16 and with fp16 operands.  masks4 is pre-filled with a fixed NaN pattern, so the planes the kernel
leaves alone hash the same in every build.  Prints one `sha256  case` line per case; with DIR the four buffers are saved there as .npy."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from saber_amd import _lib  # noqa: E402

P, DIV = 64, 8
CANARY = 0x7FC5A5A5


def main(out_dir):
    lib = _lib.load()
    assert lib.saber_k_init(0) == 0, lib.saber_k_last_error()
    g = torch.Generator(device="cuda").manual_seed(20240607)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    X = r(P, 4096, 256)
    fs1, fs0, hyper = r(P // DIV, 16384, 64), r(P // DIV, 65536, 32), r(P, 4, 32)
    w0, b0, w3, b3, lg, lb = r(256, 64, 2, 2) / 16, r(64) * 0.1, r(64, 32, 2, 2) / 8, r(32) * 0.1, 1 + 0.1 * r(64), 0.1 * r(64)
    iou4 = torch.rand(P, 4, device="cuda", generator=g)
    for op, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        prev = lib.saber_k_set_operand_type(1 if op == "fp16" else 0)
        Xo = X.to(dt).contiguous()
        for multimask in (1, 0):
            out = torch.full((P, 4, 65536), CANARY, dtype=torch.int32, device="cuda")
            st = lib.saber_k_dec_upscale(ptr(Xo), ptr(w0), ptr(b0), ptr(lg), ptr(lb), ptr(w3), ptr(b3), ptr(fs1), ptr(fs0), DIV, 0, ptr(hyper), ptr(out), P, None,
                                         ptr(iou4), multimask, None, None)
            assert st == 0, lib.saber_k_last_error().decode()
            torch.cuda.synchronize()
            a = out.cpu().numpy()
            case = f"masks4_{op}_{'multimask' if multimask else 'single'}"
            print(hashlib.sha256(a.tobytes()).hexdigest(), case, f"(written planes {int((a != CANARY).any(2).sum())} of {4 * P})")
            if out_dir:
                os.makedirs(out_dir, exist_ok=True)
                np.save(os.path.join(out_dir, case + ".npy"), a)
        lib.saber_k_set_operand_type(prev)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
