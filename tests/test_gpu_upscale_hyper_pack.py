"""The hypernetwork operand of dec_upscale_kernel, packed once per prompt (csrc/decoder_fused.hip: hyper_pack_kernel; include/saber_amd_kernels.h:
saber_k_hyper_pack), and the kernel's use of it.

hyper [P][4][32] fp32 enters the hypernetwork MFMA as hi = round(v) and lo = round(v - hi) in the 16-bit operand type; the pack kernel writes
both halves in the MFMA's k-slot order, out[p][half][m][fg][j] = channel 4 fg + j (j < 4) | 16 + 4 fg + (j - 4), and carries the overflow
sentinel's scan of hyper (the count launch_nonfinite_scan gives: one per scanning lane that met a NaN / inf).

* the pack against a torch restatement, bit for bit (tests/op16.py rounds);
* the lo half inside dec_upscale_kernel: out(h) - out(hi(h)) against out(lo(h)), which is only right when every lo value meets the u2 value
  of its own channel;
* CPU: the kernel still fits three waves per SIMD (register metadata of both operand-type builds)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.op16 import DTYPE, OPS, operand_type, rnd

CANARY = 0x7FC5A5A5


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def kcall(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the pack, bit for bit
def split_ref(h, op):
    """hi, lo of h (fp32, CPU) as the kernel computes them: hi = round(h), lo = round(h - hi); fp32 values"""
    hi = rnd(h, op)
    return hi, rnd(h - hi, op)


def pack_ref(h, op):
    """the table [P][2][4][4][8] as uint16 bit patterns (numpy) and the mask of its NaN elements"""
    P = h.shape[0]
    halves = []
    for v in split_ref(h, op):
        # [P][4][32] -> [P][4][half][fg][j'] -> [P][4][fg][half][j'] -> [P][4][fg][8]
        halves.append(v.view(P, 4, 2, 4, 4).permute(0, 1, 3, 2, 4).reshape(P, 4, 4, 8))
    t = torch.stack(halves, 1)
    return t.to(DTYPE[op]).view(torch.int16).numpy().view(np.uint16), torch.isnan(t).numpy()


def scan_count(h):
    """what launch_nonfinite_scan(h, h.numel(), counter) adds: the 4-value groups are dealt round-robin to grid x 256 lanes (grid = the groups
    / 2048 rounded up, at most 2048), and every lane that met a NaN / inf counts once"""
    bad = (~torch.isfinite(h.reshape(-1, 4))).any(1).numpy()
    lanes = 256 * min(2048, max(1, -(-bad.size // 2048)))
    return len({int(i) % lanes for i in np.nonzero(bad)[0]})


def pack_inputs(P, op, seed):
    """random hyper with the rows that matter: exactly representable values (lo = 0), magnitudes at which lo - and, with fp16, hi - is a
    denormal of the operand type or of fp32, signed zeros"""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(P, 4, 32, generator=g)
    h[0, 1] = rnd(h[0, 1], op)                       # lo exactly 0
    h[0, 2, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 0.5, 2.0 ** -14, 2.0 ** -24, 65504.0])
    h[1, 0] *= 2.0 ** -6                             # fp16: lo below 2^-14, a denormal half
    h[1, 1] *= 2.0 ** -13                            # fp16: hi around the smallest normal half, lo in its last denormal bits or 0
    h[1, 2] *= 2.0 ** -22                            # fp16: hi denormal or 0
    h[1, 3] *= 2.0 ** -120                           # bf16: lo below 2^-126, a denormal bf16 (and a denormal fp32 difference)
    h[2, 0] *= 2.0 ** -126                           # fp32 inputs at the edge of the normal range
    h[2, 1] *= 2.0 ** -135                           # denormal fp32 inputs
    h[2, 2] *= 2.0 ** 12                             # fp16: some values round to +-inf (hi), finite inputs: the counter stays
    return h


def run_pack(lib, h, op, counter0):
    P = h.shape[0]
    out = torch.full((P, 2, 4, 4, 8), 0x5A5A, dtype=torch.int16, device="cuda")
    cnt = torch.full((1,), counter0, dtype=torch.int32, device="cuda")
    hd = h.cuda().contiguous()
    with operand_type(lib, op):
        kcall(lib, lib.saber_k_hyper_pack(ptr(hd), P, ptr(out), ptr(cnt), None))
    return out.cpu().numpy().view(np.uint16), int(cnt.item())


def check_pack(lib, h, op, counter0=7):
    got, cnt = run_pack(lib, h, op, counter0)
    ref, ref_nan = pack_ref(h, op)
    got_nan = torch.isnan(torch.from_numpy(got.view(np.int16)).view(DTYPE[op]).float()).numpy()
    # a NaN is a NaN (its sign and payload are the hardware's); every other element bit for bit
    assert (got_nan == ref_nan).all(), ("NaN elements differ", np.argwhere(got_nan != ref_nan)[:5].tolist())
    diff = (got != ref) & ~ref_nan
    assert not diff.any(), (op, "elements that differ (p, half, m, fg, j): got, expected",
                            [(i.tolist(), hex(got[tuple(i)]), hex(ref[tuple(i)])) for i in np.argwhere(diff)[:8]])
    assert cnt == counter0 + scan_count(h), (op, "sentinel counter", cnt, counter0, scan_count(h))
    return cnt - counter0


@pytest.mark.gpu
@pytest.mark.parametrize("P", [5, 131])          # 131: three blocks of 256 lanes for 4192 groups: the stride loop, a ragged last round
@pytest.mark.parametrize("op", OPS)
def test_hyper_pack_is_exact(gpu_lib, op, P):
    h = pack_inputs(P, op, 1000 + P)
    hi, lo = split_ref(h, op)
    assert (lo[0, 1] == 0).all() and (lo != 0).any()
    tiny = 2.0 ** -14 if op == "fp16" else 2.0 ** -126
    n_den = int(((lo != 0) & (lo.abs() < tiny)).sum())
    assert n_den >= 16, n_den                       # denormal-range lo parts are in the case
    assert torch.isfinite(h).all() and check_pack(gpu_lib, h, op) == 0
    print(f"hyper_pack [{op}] P {P}: {n_den} denormal lo values, {int((lo == 0).sum())} zero lo values, {int(torch.isinf(hi).sum())} hi values rounded to inf")


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_hyper_pack_counts_nonfinite_as_the_scan_does(gpu_lib, op):
    P = 5
    h = pack_inputs(P, op, 77)
    a = h.clone()
    a[3, 2, 9] = float("-inf")
    a[4, 0, 30] = float("nan")
    assert check_pack(gpu_lib, a, op) == 2           # two 4-value groups, two lanes
    b = h.clone()
    b[2, 3, 4] = float("inf")
    b[2, 3, 7] = float("nan")
    assert check_pack(gpu_lib, b, op) == 1           # one group: its lane counts once
    c = torch.randn(131, 4, 32, generator=torch.Generator().manual_seed(78))
    c[0, 0, 0] = float("inf")                        # groups 0 and 768 belong to the same lane of the three-block grid
    c[24, 0, 1] = float("nan")
    c[130, 3, 31] = float("-inf")
    assert check_pack(gpu_lib, c, op) == 2
    # no counter: the table alone
    out = torch.zeros(P, 2, 4, 4, 8, dtype=torch.int16, device="cuda")
    with operand_type(gpu_lib, op):
        kcall(gpu_lib, gpu_lib.saber_k_hyper_pack(ptr(a.cuda()), P, ptr(out), None, None))
    ref, ref_nan = pack_ref(a, op)
    assert ((out.cpu().numpy().view(np.uint16) == ref) | ref_nan).all()


# ------------------------------------------------------------------------------------------------ the lo half inside dec_upscale_kernel
# fp32 accumulation is the only difference between out(h) - out(hi) and out(lo).  Per pixel the kernel computes S = MFMA(hi, u2, 0) and then
# MFMA(lo, u2, S): 32 products hi_k u2_k or lo_k u2_k, each exact in fp32 (two 16-bit significands), added to the accumulator.  u2 does not
# depend on hyper, so the three runs see the same u2 bits, S is the same bits in the runs with h and with hi(h) (where lo = 0 adds exact
# zeros), and what remains are the roundings of the lo pass on top of S in the run with h - 32 additions - and of the 32 additions of the
# run with lo(h).  Whatever the matrix core's summation order and rounding mode, one addition is off by at most one ulp of its partial sum:
# eps_fp32 |partial|.  The partial sums of the first are within max |out(h)| (1 + 2^-8), those of the second 2^-8 of that or less, so
#     |(out(h) - out(hi)) - out(lo)|  <=  32 eps (1 + 2^-8) (1 + 2^-8) max |out(h)|  <  64 eps max |out(h)|.
# A lo value in a wrong k-slot, mask row or prompt changes out(h) by the order of out(lo) itself, whose largest pixel is about 80 (bf16: |lo| up to
# 2^-9 |h|) or 10 (fp16: 2^-12) times the bound; the test requires 4 times before it asserts.
LO_MULTIPLE = 64


@pytest.mark.gpu
@pytest.mark.parametrize("P", [3, 5])
@pytest.mark.parametrize("op", OPS)
def test_lo_half_reaches_the_product_in_the_right_slots(gpu_lib, op, P):
    """86 tiles x P units on the device's workgroups: the range bounds fall inside tiles, prompts of one tile are split between workgroups;
    slot_div = 2: the walk crosses a crop; iou4 null: all four planes.

    Largest |(out(h) - out(hi)) - out(lo)| measured on an MI355X, in units of eps max |out(h)| (the bound is 64): bf16 1.13 (P = 3), 1.04 (P = 5);
    fp16 1.08 (P = 3), 1.12 (P = 5).  max |out(h)| 24.9-28.0, max |out(lo)| 5.3e-2 (bf16), 6.2-6.9e-3 (fp16) = 1.7e4 / 2.1e3 eps max |out(h)|."""
    lib, div = gpu_lib, 2
    g = torch.Generator(device="cuda").manual_seed(4200 + P)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    ns = (P - 1) // div + 1
    X = r(P, 4096, 256).to(DTYPE[op]).contiguous()
    fs1, fs0 = r(ns, 16384, 64), r(ns, 65536, 32)
    w0, b0, w3, b3, lg, lb = r(256, 64, 2, 2) / 16, r(64) * 0.1, r(64, 32, 2, 2) / 8, r(32) * 0.1, 1 + 0.1 * r(64), 0.1 * r(64)
    h = r(P, 4, 32)
    hi = rnd(h, op)
    lo = rnd(h - hi, op)
    assert (rnd(hi, op) == hi).all() and (rnd(lo, op) == lo).all() and (lo != 0).float().mean() > 0.9

    def run(hyper):
        out = torch.full((P, 4, 65536), CANARY, dtype=torch.int32, device="cuda")
        with operand_type(lib, op):
            kcall(lib, lib.saber_k_dec_upscale(ptr(X), ptr(w0), ptr(b0), ptr(lg), ptr(lb), ptr(w3), ptr(b3), ptr(fs1), ptr(fs0), div, 0, ptr(hyper.contiguous()),
                                               ptr(out), P, None, None, 0, None, None))
        assert not (out == CANARY).any(), "pixels left unwritten"
        o = out.view(torch.float32)
        assert torch.isfinite(o).all()
        return o.double()

    o_h, o_hi, o_lo = run(h), run(hi), run(lo)
    eps = float(np.finfo(np.float32).eps)
    scale = o_h.abs().max().item()
    dev = ((o_h - o_hi) - o_lo).abs()
    worst = dev.max().item()
    print(f"lo half [{op}] P {P}: max |out(h)| {scale:.3f}, max |out(lo)| {o_lo.abs().max().item():.3e}, max deviation {worst:.3e} = "
          f"{worst / (eps * scale):.2f} eps max|out(h)| (bound {LO_MULTIPLE}); per prompt {[f'{v:.2f}' for v in (dev.amax((1, 2)) / (eps * scale)).tolist()]}")
    assert o_lo.abs().max().item() > 4 * LO_MULTIPLE * eps * scale, "the lo contribution does not stand clear of the bound"
    assert worst <= LO_MULTIPLE * eps * scale, (op, P, worst, LO_MULTIPLE * eps * scale)


# ------------------------------------------------------------------------------------------------ three waves per SIMD (CPU)
@pytest.mark.parametrize("ns", ["op_bf16", "op_f16"])
def test_dec_upscale_fits_three_waves_per_simd(tmp_path_factory, ns):
    """512 VGPRs per SIMD lane / 3 waves = 170, allocated in blocks of 8: 168.  Register metadata of dec_upscale_kernel in the assembly of
    csrc/decoder_fused.hip built with the Makefile's flags (the compile is shared with tests/test_agpr_ownership.py)."""
    import re
    from tests.test_agpr_ownership import _asm
    text = _asm(ns, tmp_path_factory)
    meta = text[text.index("amdhsa.kernels:"):]
    entries = [e for e in re.split(r"^  - (?=\.)", meta, flags=re.M) if re.search(r"^\s+\.name:\s+\S*18dec_upscale_kernelE", e, re.M)]
    assert len(entries) == 1, len(entries)
    field = lambda k: int(re.search(r"^\s+\." + k + r":\s+(\d+)\s*$", entries[0], re.M).group(1))
    print(ns, {k: field(k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count")})
    assert field("vgpr_count") <= 168
    assert field("vgpr_spill_count") == 0
    assert field("sgpr_spill_count") == 0
