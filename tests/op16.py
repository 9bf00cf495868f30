"""The two 16-bit operand types of the kernel build (csrc/common.h "OPERAND TYPE": every file of the Makefile's OP_SRCS is compiled once into
namespace op_bf16 and once into op_f16; saber_k_set_operand_type picks the build for the kernel-level entry points of the calling thread).

Shared by the kernel tests: rounding to a type, the uint16 bit patterns the C-ABI takes and returns, the switch of the operand type, and the
rule the fp16 bounds of those tests follow (check_bound).  A plain module, imported as `from tests.op16 import ...`."""
import contextlib

import torch

OPS = ("bf16", "fp16")
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}            # unit roundoff (half an ulp at 1) of the type under round-to-nearest-even
DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
FP16_MAX = 65504.0
FP16_OVERFLOW = 65520.0                                # the smallest |x| that rounds to inf in IEEE half (RNE)


def rnd(x, op):
    """x rounded to the operand type (RNE, fp16 overflow to +-inf), returned as fp32 on x's device"""
    return x.to(DTYPE[op]).float()


def to_dev(x, op, device="cuda"):
    """the operand type's bit patterns of x as a uint16 tensor on `device` (what the C-ABI's uint16_t* operands take)"""
    return x.to(DTYPE[op]).view(torch.uint16).to(device)


def from_dev(t, op):
    """16-bit bit patterns (uint16 / int16 storage, or a tensor of the type itself) -> fp32 values on the CPU"""
    if t.dtype in (torch.uint16, torch.int16):
        t = t.view(DTYPE[op])
    return t.cpu().float()


@contextlib.contextmanager
def operand_type(lib, op):
    """saber_k_set_operand_type for the body of the with-statement; the previous setting comes back on exit, also on an exception"""
    prev = lib.saber_k_set_operand_type(1 if op == "fp16" else 0)
    try:
        yield
    finally:
        lib.saber_k_set_operand_type(prev)


def params(argnames, rows, ops=OPS):
    """pytest parameters of a test over the operand types: the bf16 case keeps the id the test had before it took an operand type
    (the values joined by '-'), the fp16 case carries an 'fp16-' prefix.  argnames gain a leading 'op'."""
    import pytest
    names = ["op"] + [n.strip() for n in argnames.split(",")]
    out = []
    for op in ops:
        for r in rows:
            r = tuple(r) if isinstance(r, (tuple, list)) else (r,)
            base = "-".join(str(v) for v in r)
            out.append(pytest.param(op, *r, id=base if op == "bf16" else f"fp16-{base}"))
    return ",".join(names), out


def check_bound(op, what, err, bound_bf16, bound_fp16=None, sep=None):
    """Assert err < the case's bound and print both.  bound_fp16 None: a bound set by fp32 accumulation, the same for both types.
    Otherwise it is set by a 16-bit rounding: the fp16 bound is at most 1/4 of the bf16 one and - `sep`, the same error measure of
    bf16(ref) against ref over the same case - smaller than what one bf16 rounding of the result would cost, so that an fp16 build
    that rounds through bf16 anywhere visible fails it."""
    b = bound_bf16 if (op == "bf16" or bound_fp16 is None) else bound_fp16
    tail = "" if sep is None or op == "bf16" else f", one bf16 rounding of the reference {sep:.3e}"
    print(f"{what} [{op}]: {err:.3e} (bound {b:.3e}{tail})")
    if op == "fp16" and bound_fp16 is not None:
        assert bound_fp16 <= bound_bf16 / 4, (what, bound_fp16, bound_bf16)
        assert sep is not None and bound_fp16 < sep, (what, "the fp16 bound does not tell fp16 from bf16", bound_fp16, sep)
    assert err < b, (what, op, err, b)
