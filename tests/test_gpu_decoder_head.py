"""GPU: the head of the mask decoder, kernel by kernel (include/saber_amd_kernels.h: saber_k_dec_upscale, saber_k_mask_pick,
saber_k_mask_select, saber_k_iou_live_flags).

dec_upscale_kernel (csrc/decoder_fused.hip) against a plain fp64 torch restatement of output_upscaling + the hypernetwork product, written out
below: the error is the maximum over every pixel of every compared plane, per prompt, never an RMS - a wrong 16-token tile, slot or prompt
is a few hundred pixels that are off by the size of the logits.  The bound of a case comes from the reference alone (head_bounds): what
the kernel's two documented 16-bit roundings cost (E_round), the fitted GELU's documented error (E_gelu) and fp32 accumulation (E_f32).
The engine-order layouts of X / feat_s1 / feat_s0 are built here from saber_k_perm_index alone.  masks4 is pre-filled with a NaN of a fixed
bit pattern, so "written" and "not written" are decidable per pixel; the pruned (iou4), skipped (live) and repeated runs are compared bit
for bit with the plain run of the same inputs, which is the one the reference checks.

The selection kernels are fp32 in and out: exact comparisons with a numpy restatement of oracle/sam2_ref.py's _stability + first-maximum
argmax, on planes constructed by count."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.op16 import DTYPE, OPS, check_bound, operand_type, rnd

pytestmark = pytest.mark.gpu

CANARY = 0x7FC5A5A5          # a quiet NaN no arithmetic produces (the hardware's default NaN is 0x7FC00000)
LN_EPS = 1e-6                # dec_upscale_kernel's LayerNorm2d epsilon (sam2 LayerNorm2d default)
GELU_ABS = 2.6e-5            # documented absolute error of the fitted GELU (csrc/common.h gelu_erf)
UP_TILES = 86                # 48-token tiles of the 4096 tokens (85 x 48 + 16), csrc/decoder_fused.hip


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def kcall(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()
    torch.cuda.synchronize()


_PERM = {}


def perm_grid(lib, stage, device):
    """idx[y][x] = engine row of pixel (y, x) of the stage's grid (256 >> stage), from saber_k_perm_index alone"""
    if stage not in _PERM:
        g = 256 >> stage
        idx = np.array([[lib.saber_k_perm_index(y, x, stage) for x in range(g)] for y in range(g)], dtype=np.int64)
        assert sorted(idx.ravel().tolist()) == list(range(g * g))
        _PERM[stage] = torch.from_numpy(idx.ravel())
    return _PERM[stage].to(device)


def to_engine_order(nchw, idx):
    """[n][C][g][g] -> [n][g*g][C] channels-last with pixel (y, x) in row idx[y*g + x]"""
    n, Cc, g, _ = nchw.shape
    out = torch.empty(n, g * g, Cc, dtype=nchw.dtype, device=nchw.device)
    out[:, idx] = nchw.permute(0, 2, 3, 1).reshape(n, g * g, Cc)
    return out


def n_slots(P, div, off):
    return (P - 1 + off) // div + 1


def make_inputs(P, div, off, kind, device):
    """Seeded inputs of a case in reference (NCHW, checkpoint) layout, fp32, not yet rounded.  kind: 'unit' = X, features and hyper ~ N(0, 1)
    (largest |logit| 24-30); 'big' = the same with hyper scaled afterwards so that the largest reference logit is 30 (head_case); 'small' = X rows
    LayerNorm-normalised over the channels (what the two-way transformer's final LayerNorm hands over) and hyper scaled down by 2^-5: |logit| < 1."""
    g = torch.Generator(device=device).manual_seed(10007 * P + 101 * div + off + {"unit": 0, "big": 1, "small": 2}[kind])
    r = lambda *s: torch.randn(*s, device=device, generator=g)
    ns = n_slots(P, div, off)
    d = dict(P=P, div=div, off=off, src=r(P, 256, 64, 64), f1=r(ns, 64, 128, 128), f0=r(ns, 32, 256, 256), hyper=r(P, 4, 32),
             w0=r(256, 64, 2, 2) / 16, b0=r(64) * 0.1, w3=r(64, 32, 2, 2) / 8, b3=r(32) * 0.1, lg=1 + 0.1 * r(64), lb=0.1 * r(64))
    # plane 0 of every odd prompt is small (2^-7: exact), so that its stability score falls below 0.98 and the selection kernels that run on
    # this kernel's output take the "best of planes 1-3" branch for those prompts and the "plane 0" branch for the others
    d["hyper"][1::2, 0] *= 2.0 ** -7
    if kind == "small":
        s = d["src"]
        d["src"] = (s - s.mean(1, keepdim=True)) / s.var(1, unbiased=False, keepdim=True).add(1e-5).sqrt()
        d["hyper"] *= 2.0 ** -5
    return d


def gelu(x):
    return F.gelu(x)          # approximate='none': the exact erf form


def head_ref(d, op, dt, emulate, p0, p1):
    """masks4[p0:p1] of the upscaling head in dtype dt from the operands the kernel gets (X, w0, w3 rounded to the operand type, everything
    else fp32 widened).  emulate: the kernel's two 16-bit roundings (the GELU output of phase A = B operand of the second ConvT, and u2
    before the hypernetwork MFMA; csrc/decoder_fused.hip "epilogue A" / UP_MFMA_HYPER) are applied."""
    q = (lambda t: rnd(t.float(), op).to(dt)) if emulate else (lambda t: t)
    sl = (torch.arange(p0, p1, device=d["src"].device) + d["off"]) // d["div"]
    x = F.conv_transpose2d(rnd(d["src"][p0:p1], op).to(dt), rnd(d["w0"], op).to(dt), d["b0"].to(dt), stride=2) + d["f1"][sl].to(dt)
    mu = x.mean(1, keepdim=True)
    var = (x - mu).pow(2).mean(1, keepdim=True)
    x = (x - mu) / (var + LN_EPS).sqrt() * d["lg"].to(dt)[None, :, None, None] + d["lb"].to(dt)[None, :, None, None]
    x = q(gelu(x))
    y = F.conv_transpose2d(x, rnd(d["w3"], op).to(dt), d["b3"].to(dt), stride=2) + d["f0"][sl].to(dt)
    y = q(gelu(y))
    return torch.einsum("pkc,pchw->pkhw", d["hyper"][p0:p1].to(dt), y)


def head_bounds(d, op, chunk=8):
    """The fp64 reference of a case and the three terms of its bound, per prompt (module docstring).  Returns ref [P][4][256][256] fp64,
    emul (the same with the kernel's roundings emulated) fp32, and E_round, E_gelu, E_f32, scale (largest |reference logit|), sep (one bf16
    rounding of the reference, normalised)."""
    P = d["P"]
    dev = d["src"].device
    ref = torch.empty(P, 4, 256, 256, dtype=torch.float64, device=dev)
    emul = torch.empty(P, 4, 256, 256, dtype=torch.float32, device=dev)
    e_round = torch.empty(P, dtype=torch.float64, device=dev)
    e_f32 = torch.empty(P, dtype=torch.float64, device=dev)
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):      # the native col2im + GEMM path: fp64 is supported, fp32 is one plain summation order
        for p0 in range(0, P, chunk):
            p1 = min(P, p0 + chunk)
            r = head_ref(d, op, torch.float64, False, p0, p1)
            e = head_ref(d, op, torch.float64, True, p0, p1)
            f = head_ref(d, op, torch.float32, False, p0, p1)
            ref[p0:p1] = r
            emul[p0:p1] = e.float()
            e_round[p0:p1] = (e - r).abs().amax((1, 2, 3))
            e_f32[p0:p1] = (f.double() - r).abs().amax((1, 2, 3))
    w3sum = rnd(d["w3"], op).double().abs().sum(0).max()                  # max over the outputs (co, dy, dx) of sum_ci |w3|
    e_gelu = GELU_ABS * (1 + w3sum) * d["hyper"].double().abs().sum(2).amax(1)
    scale = ref.abs().amax((1, 2, 3))
    sep = (rnd(ref.float(), "bf16").double() - ref).abs().amax((1, 2, 3)) / scale
    return dict(ref=ref, emul=emul, E_round=e_round, E_gelu=e_gelu, E_f32=e_f32, scale=scale, sep=sep)


def bound_of(b):
    """bound[p] = 2 E_round + E_gelu + 8 E_f32: the kernel rounds at slightly different values than the emulation, so its rounding error is
    another draw of the same size and a maximum over 262 144 pixels varies by less than 2x between draws; 8x on the fp32 term covers another
    summation order and the MFMA's"""
    return 2 * b["E_round"] + b["E_gelu"] + 8 * b["E_f32"]


_CASES = {}


def head_case(lib, P, div=None, off=0, kind="unit"):
    """inputs (reference layout + the engine-order device buffers of both operand types), reference and bounds of a case: computed once"""
    div = P if div is None else div
    key = (P, div, off, kind)
    if key in _CASES:
        return _CASES[key]
    d = make_inputs(P, div, off, kind, "cuda")
    if kind == "big":        # hyper scaled so that the largest logit of the (bf16-operand) reference is 30, the range mask_input is clamped to
        d["hyper"] *= 30.0 / head_bounds(d, "bf16")["scale"].max().float()
    c = dict(d=d, P=P, div=div, off=off, kind=kind, bounds={op: head_bounds(d, op) for op in OPS}, plain={})
    i2, i1, i0 = (perm_grid(lib, s, "cuda") for s in (2, 1, 0))
    c["X"] = {op: to_engine_order(d["src"].to(DTYPE[op]), i2).contiguous() for op in OPS}
    c["fs1"] = to_engine_order(d["f1"], i1).contiguous()
    c["fs0"] = to_engine_order(d["f0"], i0).contiguous()
    _CASES[key] = c
    return c


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_head(lib, c, op, live=None, iou4=None, multimask=0, X=None, hyper=None, sentinel=None):
    """one launch into a canary-filled masks4; returns its bits (int32 [P][4][65536]) and the sentinel counter after the call"""
    d, P = c["d"], c["P"]
    out = torch.full((P, 4, 65536), CANARY, dtype=torch.int32, device="cuda")
    sent = torch.zeros(1, dtype=torch.int32, device="cuda") if sentinel is None else sentinel
    X = c["X"][op] if X is None else X
    hyper = d["hyper"] if hyper is None else hyper
    assert X.is_contiguous() and hyper.is_contiguous()
    with operand_type(lib, op):
        kcall(lib, lib.saber_k_dec_upscale(ptr(X), ptr(d["w0"]), ptr(d["b0"]), ptr(d["lg"]), ptr(d["lb"]), ptr(d["w3"]), ptr(d["b3"]), ptr(c["fs1"]), ptr(c["fs0"]),
                                           c["div"], c["off"], ptr(hyper), ptr(out), P, ptr(live), ptr(iou4), multimask, ptr(sent), None))
    return out, int(sent.item())


def plain_run(lib, c, op):
    """the run without live / iou4 (every plane of every prompt), cached: what the pruned and skipped runs are compared with bit for bit"""
    if op not in c["plain"]:
        out, sent = run_head(lib, c, op)
        assert sent == 0, "overflow sentinel raised on finite inputs"
        c["plain"][op] = out
    return c["plain"][op]


def is_canary(bits):
    return bits == CANARY


def check_against_reference(lib, c, op, what):
    """every pixel of all four planes of every prompt against fp64, per prompt, through check_bound (normalised by the prompt's largest |logit|)"""
    P = c["P"]
    units = UP_TILES * P
    print(f"{what} [{op}]: P {P}, slot map (div {c['div']}, off {c['off']}), units {units}, grid {min(units, n_cu())} of {n_cu()} CUs")
    out = plain_run(lib, c, op)
    assert not is_canary(out).any(), "pixels left unwritten"
    got = out.view(torch.float32).view(P, 4, 256, 256)
    assert torch.isfinite(got).all()
    b, bb, bf = c["bounds"][op], c["bounds"]["bf16"], c["bounds"]["fp16"]
    err = (got.double() - b["ref"]).abs().amax((1, 2, 3))
    vs_emul = (got - b["emul"]).abs().amax((1, 2, 3))
    bound = bound_of(b)
    worst = int((err / bound).argmax())
    print(f"  worst prompt {worst}: err {err[worst]:.3e} = {err[worst] / bound[worst]:.2f} of the bound {bound[worst]:.3e} (E_round {b['E_round'][worst]:.3e}, "
          f"E_gelu {b['E_gelu'][worst]:.3e}, E_f32 {b['E_f32'][worst]:.3e}); largest |logit| {b['scale'][worst]:.2f}; |kernel - emulated| {vs_emul[worst]:.3e}; "
          f"max err / bound over the prompts {(err / bound).max():.3f}")
    nb, nf = bound_of(bb) / bb["scale"], bound_of(bf) / bf["scale"]
    for p in sorted({0, P - 1, worst, int(nf.argmax()), int((nf / nb).argmax()), int((nf / bf["sep"]).argmax())}):
        check_bound(op, f"  {what} prompt {p}: max |kernel - fp64| / max |logit|", (err[p] / b["scale"][p]).item(), nb[p].item(), nf[p].item(), bf["sep"][p].item())
    # every prompt (check_bound above prints a few and checks the fp16 rule where it is tightest)
    assert (nf <= nb / 4).all() and (nf < bf["sep"]).all(), "the fp16 bound does not tell fp16 from bf16 for some prompt"
    # largest measured err / bound over all cases of this module on an MI355X: 0.62 with bf16 operands, 0.45 with fp16 operands
    assert (err < bound).all(), (what, op, "prompts over their bound", torch.nonzero(err >= bound).flatten().tolist()[:10], (err / bound).max().item())
    return (err / bound).max().item()


# ------------------------------------------------------------------------------------------------ dec_upscale against fp64
# 86 P units against the CUs (256 on an MI355X): 86 and 172 = one unit per workgroup; 258 = ranges of one and two units that change prompt
# inside a tile; 602 = two or three; 5504 / 5762 / 11 266 = ranges that start and end mid-tile
@pytest.mark.parametrize("P", [1, 2, 3, 7, 64, 67, 131])
@pytest.mark.parametrize("op", OPS)
def test_dec_upscale_every_pixel(gpu_lib, op, P):
    """all four planes of every prompt, no live / iou4: no canary left, max over all pixels per prompt inside the bound computed from the
    reference (check_against_reference)"""
    r = check_against_reference(gpu_lib, head_case(gpu_lib, P), op, "dec_upscale")
    print(f"dec_upscale P {P} [{op}]: largest err / bound {r:.3f}")


@pytest.mark.parametrize("div,off", [(1, 0), (0, 0), (3, 2), (64, 37)])      # div 0 stands for div = P (one slot for all)
@pytest.mark.parametrize("P", [7, 131])
@pytest.mark.parametrize("op", OPS)
def test_dec_upscale_slot_maps(gpu_lib, op, P, div, off):
    """prompt p reads the features of slot (p + off) / div, every slot with its own random features: a prompt that reads a neighbour's
    features is off by O(1)"""
    check_against_reference(gpu_lib, head_case(gpu_lib, P, div or P, off), op, "dec_upscale slots")


@pytest.mark.parametrize("kind", ["big", "small"])
@pytest.mark.parametrize("op", OPS)
def test_dec_upscale_magnitudes(gpu_lib, op, kind):
    """the normalised bound where the logits are large (hyper scaled so that they reach +-30, the range mask_input is clamped to) and where
    they are small (X of LayerNorm scale, small hyper)"""
    c = head_case(gpu_lib, 3, kind=kind)
    print(f"largest |logit| per prompt: {c['bounds'][op]['scale'].tolist()}")
    check_against_reference(gpu_lib, c, op, f"dec_upscale {kind} logits")


# ------------------------------------------------------------------------------------------------ pruning, skipping, repeatability: bit for bit
def first_max(row):
    """1 + index of the first maximum of row[1:4] by the kernels' rule: start at plane 1, move on only for a strictly greater value (a NaN
    never wins and, once held, is never beaten).  Equals 1 + numpy.argmax(row[1:]) for rows without NaN."""
    best, bv = 1, row[1]
    for k in (2, 3):
        if row[k] > bv:
            best, bv = k, row[k]
    return best


def tie_rows(P, seed):
    """iou4 [P][4] float32: random rows, then the ties and edge values the tie rule must get right"""
    rng = np.random.default_rng(seed)
    iou = rng.uniform(0.05, 0.95, (P, 4)).astype(np.float32)
    a, b = np.float32(0.75), np.float32(0.5)
    tiny = np.float32(1e-45)                      # the smallest denormal
    special = [(a, a, b), (b, a, a), (a, a, a), (a, b, a), (0, 0, 0), (1, 1, 1), (0, 1, 1), (1, 0, 1), (0, 0, 1), (tiny, 0, tiny), (0, tiny, tiny),
               (2 * tiny, tiny, 2 * tiny), (a, np.nextafter(a, np.float32(1)), np.nextafter(a, np.float32(1))), (-0.0, 0.0, 0.0), (0.0, -0.0, 0.0)]
    spread = P > 5 * len(special)                 # large P: the special rows lie apart, so that they fall into different workgroups' ranges
    for i, s in enumerate(special[:P]):
        iou[5 * i + 1 if spread else i, 1:] = s
    return iou


def expect_planes(out, plain, need_of, what):
    """plane k of prompt p is bit-identical to the plain run where need_of(p) has bit k, and holds the canary in every pixel elsewhere"""
    P = out.shape[0]
    need = torch.tensor([[bool((need_of(p) >> k) & 1) for k in range(4)] for p in range(P)], device=out.device)
    same = (out == plain).all(2)
    untouched = is_canary(out).all(2)
    bad_w = torch.nonzero(need & ~same).tolist()
    bad_u = torch.nonzero(~need & ~untouched).tolist()
    assert not bad_w, (what, "planes that differ from the plain run (prompt, plane)", bad_w[:10])
    assert not bad_u, (what, "planes written that nobody asked for (prompt, plane)", bad_u[:10])


@pytest.mark.parametrize("P", [7, 67, 131])
@pytest.mark.parametrize("op", OPS)
def test_dec_upscale_iou4_multimask_skips_plane_0(gpu_lib, op, P):
    c = head_case(gpu_lib, P)
    iou = torch.from_numpy(tie_rows(P, 3)).cuda()
    out, sent = run_head(gpu_lib, c, op, iou4=iou, multimask=1)
    expect_planes(out, plain_run(gpu_lib, c, op), lambda p: 0xE, "multimask")
    assert sent == 0


@pytest.mark.parametrize("P", [7, 67, 131])
@pytest.mark.parametrize("op", OPS)
def test_dec_upscale_iou4_single_mask_writes_what_the_selection_reads(gpu_lib, op, P):
    """single-mask mode with iou4: exactly plane 0 and plane 1 + argmax(iou4[p][1:]) (first maximum) are written, bit-identical to the plain
    run; then the chain the engine runs on it - saber_k_mask_pick chooses a plane that holds no canary pixel for every prompt (stable and
    unstable plane 0 alternate: make_inputs) and saber_k_mask_select copies no canary."""
    c = head_case(gpu_lib, P)
    iou_h = tie_rows(P, 5)
    assert all(first_max(r) == 1 + int(np.argmax(r[1:])) for r in iou_h)
    iou = torch.from_numpy(iou_h).cuda()
    out, sent = run_head(gpu_lib, c, op, iou4=iou, multimask=0)
    plain = plain_run(gpu_lib, c, op)
    expect_planes(out, plain, lambda p: 1 | (1 << first_max(iou_h[p])), "single mask")
    assert sent == 0
    check_selection_chain(gpu_lib, out, plain, iou, iou_h, None)


def check_selection_chain(lib, out, plain, iou, iou_h, live_h):
    P = out.shape[0]
    m4 = out.view(torch.float32)
    sel = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    oi = torch.full((P,), -7.0, device="cuda")
    live = None if live_h is None else torch.from_numpy(live_h).cuda()
    kcall(lib, lib.saber_k_mask_pick(ptr(m4), ptr(iou), P, 0, ptr(oi), ptr(sel), ptr(live), None))
    sel_h = sel.cpu().numpy()
    r_sel, _ = select_ref(plain.view(torch.float32).view(P, 4, 65536)[:, 0].cpu().numpy(), iou_h)
    alive = np.ones(P, bool) if live_h is None else live_h.astype(bool)
    assert np.array_equal(sel_h[alive], r_sel[alive]) and (sel_h[~alive] == 0).all()
    assert len(set(sel_h[alive].tolist())) > 1 or P < 2, "the case exercises one branch of the selection only"
    chosen = out[torch.arange(P, device="cuda"), sel.long()]
    assert not is_canary(chosen[torch.from_numpy(alive).cuda()]).any(), "mask_pick chose a plane dec_upscale did not write"
    if live_h is None:
        om = torch.full((P, 65536), CANARY, dtype=torch.int32, device="cuda")
        oi2 = torch.full((P,), -7.0, device="cuda")
        kcall(lib, lib.saber_k_mask_select(ptr(m4), ptr(iou), P, 0, ptr(om.view(torch.float32)), ptr(oi2), None))
        assert not is_canary(om).any(), "mask_select copied pixels dec_upscale did not write"
        assert torch.equal(om, plain[torch.arange(P, device="cuda"), sel.long()]) and torch.equal(oi.view(torch.int32), oi2.view(torch.int32))


@pytest.mark.parametrize("op", OPS)
def test_dec_upscale_iou4_nan_rows_agree_across_the_three_kernels(gpu_lib, op):
    """NaN among iou4[p][1..3].  All three kernels run the same comparison chain (start at plane 1, move on for a strictly greater value): a
    NaN in place 2 or 3 never wins, a NaN in place 1 is never beaten - first_max above.  torch.argmax / numpy.argmax would return the first
    NaN instead, so the planes differ from the oracle's choice; what reports a NaN IoU at run time is the engine's overflow sentinel
    (launch_nonfinite_scan over iou4 before this kernel, saber_engine_check_finite), not these kernels.  Asserted here: the plane
    dec_upscale computes is the plane mask_pick picks and mask_select copies, so none of them reads memory that was not written."""
    P = 7
    c = head_case(gpu_lib, P)
    nan = np.float32(np.nan)
    iou_h = tie_rows(P, 7)
    iou_h[:, 1:] = [(nan, 0.5, 0.7), (0.5, nan, 0.7), (0.5, 0.7, nan), (nan, nan, 0.7), (0.7, nan, nan), (nan, nan, nan), (0.5, nan, 0.4)]
    iou = torch.from_numpy(iou_h).cuda()
    out, sent = run_head(gpu_lib, c, op, iou4=iou, multimask=0)
    plain = plain_run(gpu_lib, c, op)
    expect_planes(out, plain, lambda p: 1 | (1 << first_max(iou_h[p])), "NaN rows")
    assert sent == 0          # the logits are finite: this kernel's counter watches what it stores, not iou4
    # every prompt unstable (plane 0 scaled down), so that the selection goes to planes 1-3 everywhere
    hy = c["d"]["hyper"].clone()
    hy[0::2, 0] *= 2.0 ** -7
    out2, _ = run_head(gpu_lib, c, op, iou4=iou, multimask=0, hyper=hy)
    full2, _ = run_head(gpu_lib, c, op, hyper=hy)
    sel = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    oi = torch.zeros(P, device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_mask_pick(ptr(out2.view(torch.float32)), ptr(iou), P, 0, ptr(oi), ptr(sel), None, None))
    assert sel.cpu().tolist() == [first_max(r) for r in iou_h]
    om = torch.full((P, 65536), CANARY, dtype=torch.int32, device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_mask_select(ptr(out2.view(torch.float32)), ptr(iou), P, 0, ptr(om.view(torch.float32)), ptr(oi), None))
    assert not is_canary(om).any() and torch.equal(om, full2[torch.arange(P, device="cuda"), sel.long()])


def live_patterns(P, seed):
    rng = np.random.default_rng(seed)
    pats = {"random": (rng.uniform(size=P) < 0.5).astype(np.uint8)}
    pats["first dead"] = np.ones(P, np.uint8); pats["first dead"][0] = 0
    pats["last dead"] = np.ones(P, np.uint8); pats["last dead"][-1] = 0
    # 86 P units over min(86 P, CUs) workgroups: a range holds at most ceil(86 P / CUs) units, i.e. at most that many prompts of one tile
    run = min(P - 2, -(-UP_TILES * P // min(UP_TILES * P, n_cu())) + 5)
    pats[f"dead run of {run}"] = np.ones(P, np.uint8); pats[f"dead run of {run}"][1:1 + run] = 0
    pats["all dead but one"] = np.zeros(P, np.uint8); pats["all dead but one"][P // 2] = 1
    pats["all dead"] = np.zeros(P, np.uint8)
    return pats


@pytest.mark.parametrize("op", OPS)
def test_dec_upscale_live_flags(gpu_lib, op):
    """dead prompts keep the canary in all four planes, live prompts are bit-identical to the run without flags; "all dead" returns with
    nothing written (what a high pred_iou_thresh produces)"""
    P = 131
    c = head_case(gpu_lib, P)
    plain = plain_run(gpu_lib, c, op)
    for name, lv in live_patterns(P, 11).items():
        out, sent = run_head(gpu_lib, c, op, live=torch.from_numpy(lv).cuda())
        expect_planes(out, plain, lambda p: 0xF if lv[p] else 0, f"live: {name}")
        assert sent == 0
        print(f"live [{op}] {name}: {int(lv.sum())} of {P} live - ok")


@pytest.mark.parametrize("op", OPS)
def test_dec_upscale_live_with_iou4_and_slot_map(gpu_lib, op):
    P = 131
    c = head_case(gpu_lib, P, 3, 2)
    plain = plain_run(gpu_lib, c, op)
    lv = live_patterns(P, 13)["random"]
    iou_h = tie_rows(P, 17)
    iou = torch.from_numpy(iou_h).cuda()
    out, sent = run_head(gpu_lib, c, op, live=torch.from_numpy(lv).cuda(), iou4=iou, multimask=0)
    expect_planes(out, plain, lambda p: (1 | (1 << first_max(iou_h[p]))) if lv[p] else 0, "live + iou4 + slots")
    assert sent == 0
    check_selection_chain(gpu_lib, out, plain, iou, iou_h, lv)


@pytest.mark.parametrize("P", [3, 131])
@pytest.mark.parametrize("op", OPS)
def test_dec_upscale_is_run_to_run_identical(gpu_lib, op, P):
    c = head_case(gpu_lib, P)
    a, _ = run_head(gpu_lib, c, op)
    assert torch.equal(a, plain_run(gpu_lib, c, op))


@pytest.mark.parametrize("op", OPS)
def test_dec_upscale_overflow_sentinel(gpu_lib, op):
    """the counter stays 0 on finite inputs (every test above checks that); it becomes non-zero - and grows again on a second call without a
    reset - when one token of a live prompt carries +inf in X and when hyper makes a stored plane overflow fp32; non-finite values that
    belong to a dead prompt or to a plane that is not stored leave it at 0"""
    P = 3
    c = head_case(gpu_lib, P)
    X = c["X"][op].clone()
    X[1, 1234, 17] = float("inf")
    sent = torch.zeros(1, dtype=torch.int32, device="cuda")
    out, s1 = run_head(gpu_lib, c, op, X=X, sentinel=sent)
    _, s2 = run_head(gpu_lib, c, op, X=X, sentinel=sent)
    print(f"sentinel [{op}] +inf in one token of X: {s1}, after a second call {s2}")
    assert s1 > 0 and s2 > s1
    got = out.view(torch.float32).view(P, 4, 65536)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[2]).all() and not torch.isfinite(got[1]).all()
    live = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    _, s = run_head(gpu_lib, c, op, X=X, live=live)
    assert s == 0, "the non-finite token belongs to a dead prompt"
    hy = c["d"]["hyper"].clone()
    hy[2, 3] = 3.0e38
    sent.zero_()
    _, s1 = run_head(gpu_lib, c, op, hyper=hy, sentinel=sent)
    _, s2 = run_head(gpu_lib, c, op, hyper=hy, sentinel=sent)
    print(f"sentinel [{op}] plane 3 of one prompt beyond fp32: {s1}, after a second call {s2}")
    assert s1 > 0 and s2 > s1
    iou = torch.tensor([[0.5, 0.9, 0.1, 0.2]] * P, device="cuda")            # single-mask mode stores planes 0 and 1: plane 3 is not stored
    _, s = run_head(gpu_lib, c, op, hyper=hy, iou4=iou, multimask=0)
    assert s == 0, "the overflowing plane is not stored"


# ------------------------------------------------------------------------------------------------ the selection kernels (fp32, exact)
def select_ref(m0, iou4):
    """oracle/sam2_ref.py _stability (delta 0.05, threshold 0.98) + first-maximum argmax in float32 as the kernels compute it: stability =
    (float)#(m0 > 0.05f) / (float)#(m0 > -0.05f), 1 when the denominator is 0; NaN pixels are in neither count.  m0 [P][65536], iou4 [P][4]"""
    d = np.float32(0.05)
    ai = (m0 > d).sum(1).astype(np.float32)
    au = (m0 > -d).sum(1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        stab = np.where(au > 0, ai / au, np.float32(1.0)).astype(np.float32)
    sel = np.array([0 if stab[p] >= np.float32(0.98) else first_max(iou4[p]) for p in range(len(m0))], dtype=np.int32)
    return sel, iou4[np.arange(len(m0)), sel]


# (pixels > +0.05, pixels in (-0.05, +0.05]) of plane 0; the rest is <= -0.05.  stable <=> (float)ai / (float)(ai + band) >= 0.98f
COUNTS = [(49, 1), (48, 2), (65536, 0), (0, 0), (0, 7), (98, 2), (97, 3), (64226, 1310), (64225, 1311), (1, 0), (32768, 668), (32768, 669), (5, 65531)]


def plane0_by_count(ai, band, layout, rng):
    """a plane 0 with exactly `ai` pixels above +0.05 and `band` pixels inside the band, among them the edge values: exactly +0.05f (not
    above), exactly -0.05f (not inside), +-0 (inside), NaN (in neither count).  layout: where the counted pixels sit - the first float4s, the
    last float4s, or scattered - so that a reduction that drops a wave or a tail is caught."""
    d = np.float32(0.05)
    m = np.full(65536, -1.0, np.float32)
    n = ai + band
    if layout == "first":
        pos = np.arange(n)
    elif layout == "last":
        pos = 65536 - 1 - np.arange(n)
    else:
        pos = rng.permutation(65536)[:n]
    hi, mid = pos[:ai], pos[ai:]
    m[hi] = rng.uniform(0.06, 30.0, ai).astype(np.float32)
    if ai:
        m[hi[0]] = np.nextafter(d, np.float32(1))                   # the smallest value above +0.05f
    vals = np.array([d, 0.0, -0.0, np.nextafter(-d, np.float32(0)), 0.04, -0.04], np.float32)       # +0.05f itself is inside the band, not above
    m[mid] = vals[np.arange(band) % len(vals)]
    rest = np.setdiff1d(np.arange(65536), pos, assume_unique=False)
    if len(rest) >= 3:
        m[rest[0]] = -d                                             # exactly -0.05f: not > -0.05f
        m[rest[len(rest) // 2]] = np.nan
        m[rest[-1]] = np.nan
    assert (m > d).sum() == ai and (m > -d).sum() == n
    return m


def selection_inputs(P, seed):
    rng = np.random.default_rng(seed)
    m4 = rng.standard_normal((P, 4, 65536), dtype=np.float32)
    for p in range(P):
        ai, band = COUNTS[p % len(COUNTS)]
        m4[p, 0] = plane0_by_count(ai, band, ("first", "last", "scattered")[(p // len(COUNTS) + p) % 3], rng)
    if P < len(COUNTS):                                              # small P: the two sides of 49 / 50 and the empty plane
        for p, (ai, band) in enumerate([(49, 1), (48, 2), (0, 0)][:P]):
            m4[p, 0] = plane0_by_count(ai, band, ("scattered", "last", "first")[p], rng)
    return m4, tie_rows(P, seed + 1)


@pytest.mark.parametrize("P", [1, 3, 300])
def test_mask_pick_and_select_exact(gpu_lib, P):
    """single-mask mode: out_sel and out_iou of mask_pick equal the numpy restatement exactly, mask_select copies the chosen plane bit for bit
    and agrees with mask_pick on every prompt; multimask mode: iou4[:, 1:], planes 1-3, out_sel left alone; out_sel = NULL accepted"""
    m4_h, iou_h = selection_inputs(P, 100 + P)
    r_sel, r_iou = select_ref(m4_h[:, 0], iou_h)
    if P >= len(COUNTS):
        exp = [0, 1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1]        # 1 = unstable: 48/50, 0/7, 97/100, 64225/65536, 32768/33437, 5/65536 < 0.98 <= the others; au = 0 is stable
        assert [int(s != 0) for s in r_sel[:len(COUNTS)]] == exp, "the restatement itself"
    m4 = torch.from_numpy(m4_h).cuda()
    iou = torch.from_numpy(iou_h).cuda()
    sel = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    oi = torch.full((P,), -7.0, device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_mask_pick(ptr(m4), ptr(iou), P, 0, ptr(oi), ptr(sel), None, None))
    assert np.array_equal(sel.cpu().numpy(), r_sel), np.nonzero(sel.cpu().numpy() != r_sel)[0][:10]
    assert np.array_equal(oi.cpu().numpy().view(np.int32), r_iou.view(np.int32))
    oi_b = torch.full((P,), -7.0, device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_mask_pick(ptr(m4), ptr(iou), P, 0, ptr(oi_b), None, None, None))          # out_sel = NULL
    assert torch.equal(oi_b.view(torch.int32), oi.view(torch.int32))
    om = torch.full((P, 65536), CANARY, dtype=torch.int32, device="cuda")
    oi2 = torch.full((P,), -7.0, device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_mask_select(ptr(m4), ptr(iou), P, 0, ptr(om.view(torch.float32)), ptr(oi2), None))
    want = m4.view(torch.int32)[torch.arange(P, device="cuda"), torch.from_numpy(r_sel).long().cuda()]
    assert torch.equal(om, want) and torch.equal(oi2.view(torch.int32), oi.view(torch.int32))
    # multimask
    sel.fill_(-7)
    oi3 = torch.full((P, 3), -7.0, device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_mask_pick(ptr(m4), ptr(iou), P, 1, ptr(oi3), ptr(sel), None, None))
    assert torch.equal(oi3.view(torch.int32), iou[:, 1:].contiguous().view(torch.int32)) and (sel == -7).all()
    om3 = torch.full((P, 3, 65536), CANARY, dtype=torch.int32, device="cuda")
    oi4 = torch.full((P, 3), -7.0, device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_mask_select(ptr(m4), ptr(iou), P, 1, ptr(om3.view(torch.float32)), ptr(oi4), None))
    assert torch.equal(om3, m4.view(torch.int32)[:, 1:]) and torch.equal(oi4.view(torch.int32), oi3.view(torch.int32))


@pytest.mark.parametrize("P", [3, 300])
def test_mask_pick_live_prompts_only(gpu_lib, P):
    """with `live`: dead prompts give plane 0 and iou4[p][0] and their planes are never read (they are NaN here, which would change the counts)"""
    m4_h, iou_h = selection_inputs(P, 200 + P)
    lv = (np.random.default_rng(P).uniform(size=P) < 0.5).astype(np.uint8)
    lv[0], lv[-1] = 0, 1
    r_sel, r_iou = select_ref(m4_h[:, 0], iou_h)
    r_sel[lv == 0] = 0
    r_iou[lv == 0] = iou_h[lv == 0, 0]
    m4_h[lv == 0] = np.nan
    m4, iou = torch.from_numpy(m4_h).cuda(), torch.from_numpy(iou_h).cuda()
    sel = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    oi = torch.full((P,), -7.0, device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_mask_pick(ptr(m4), ptr(iou), P, 0, ptr(oi), ptr(sel), ptr(torch.from_numpy(lv).cuda()), None))
    assert np.array_equal(sel.cpu().numpy(), r_sel) and np.array_equal(oi.cpu().numpy().view(np.int32), r_iou.view(np.int32))


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000])
def test_iou_live_flags(gpu_lib, P):
    """live[p] = any of the four IoUs > thr, strictly; counters are added to over two calls and may be NULL; bytes beyond P keep their canary"""
    rng = np.random.default_rng(P)
    thr = np.float32(0.7)
    iou_h = rng.uniform(0.3, 0.8, (P, 4)).astype(np.float32)
    edge = [(thr, thr, thr, thr), (thr, 0, 0, 0), (np.nextafter(thr, np.float32(1)), 0, 0, 0), (0, 0, 0, np.nextafter(thr, np.float32(1))),
            (0, 0, np.nextafter(thr, np.float32(0)), 0), (np.nan, thr, 0, 0), (np.nan, 0.9, 0, 0)]
    for i, e in enumerate(edge):
        iou_h[(i * 37) % P] = e
    iou_h[P - 1] = (0, 0, 0, np.nextafter(thr, np.float32(1))) if P % 2 else (thr, thr, thr, thr)
    want = (iou_h > thr).any(1).astype(np.uint8)
    iou = torch.from_numpy(iou_h).cuda()
    pad = 300
    live = torch.full((P + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.tensor([5, 11], dtype=torch.int64, device="cuda")
    for rep in (1, 2):
        kcall(gpu_lib, gpu_lib.saber_k_iou_live_flags(ptr(iou), P, float(thr), ptr(live), ptr(cnt), None))
        assert np.array_equal(live[:P].cpu().numpy(), want) and (live[P:] == 0xA5).all()
        assert cnt.tolist() == [5 + rep * int((want == 0).sum()), 11 + rep * P]
    live.fill_(0xA5)
    kcall(gpu_lib, gpu_lib.saber_k_iou_live_flags(ptr(iou), P, float(thr), ptr(live), None, None))
    assert np.array_equal(live[:P].cpu().numpy(), want) and (live[P:] == 0xA5).all()
