"""CPU: the operand-type helpers the kernel tests share (tests/op16.py)."""
import pytest
import torch

from tests.op16 import FP16_MAX, FP16_OVERFLOW, OPS, U, check_bound, from_dev, operand_type, params, rnd, to_dev


def test_rounding_and_bits():
    x = torch.tensor([1.0 + 2.0 ** -9, 65519.0, FP16_OVERFLOW, -1e6, 2.0 ** -24, 3.0e-8, 1.0 / 3.0])
    assert rnd(x, "bf16").tolist()[0] == 1.0 and rnd(x, "fp16").tolist()[0] == 1.0 + 2.0 ** -9
    h = rnd(x, "fp16")
    assert h[1].item() == FP16_MAX and h[2].item() == float("inf") and h[3].item() == float("-inf")
    assert h[4].item() == 2.0 ** -24 and h[5].item() == 2.0 ** -24          # subnormals kept (3e-8 is just above half of 2^-24)
    for op in OPS:
        b = to_dev(x, op, device="cpu")
        assert b.dtype == torch.uint16
        assert torch.equal(from_dev(b, op), rnd(x, op))
        assert torch.equal(from_dev(b.view(torch.int16), op), rnd(x, op))
        assert abs(rnd(x[6:], op).item() - 1.0 / 3.0) <= U[op] / 3.0


class _FakeLib:
    def __init__(self):
        self.f16 = 0

    def saber_k_set_operand_type(self, f16):
        prev, self.f16 = self.f16, f16
        return prev


def test_operand_type_restores_on_exit_and_on_exception():
    lib = _FakeLib()
    with operand_type(lib, "fp16"):
        assert lib.f16 == 1
        with operand_type(lib, "bf16"):
            assert lib.f16 == 0
        assert lib.f16 == 1
    assert lib.f16 == 0
    with pytest.raises(RuntimeError):
        with operand_type(lib, "fp16"):
            raise RuntimeError("kernel failed")
    assert lib.f16 == 0


def test_params_keep_the_bf16_ids_and_check_bound_rules():
    names, ps = params("M,N", [(3, 4), (5, 6)])
    assert names == "op,M,N" and [p.id for p in ps] == ["3-4", "5-6", "fp16-3-4", "fp16-5-6"]
    check_bound("fp16", "ok", 1e-4, 8e-3, 1e-3, 2e-3)
    with pytest.raises(AssertionError):
        check_bound("fp16", "bound above a bf16 rounding", 1e-4, 8e-3, 1e-3, 5e-4)
    with pytest.raises(AssertionError):
        check_bound("fp16", "bound above 1/4 of the bf16 one", 1e-4, 2e-3, 1e-3, 5e-3)
    with pytest.raises(AssertionError):
        check_bound("bf16", "error above the bound", 9e-3, 8e-3, 1e-3, 2e-3)
