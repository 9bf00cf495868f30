"""GPU: the launch ledger of the 16-bit mask-decoder driver (csrc/engine.hip: decode_chunk), through the public Engine API and its per-class
launch profile (Engine.profile_begin / profile_end).

One driver body decodes a chunk of P prompts on two routes: R = 8 token rows per prompt (one point: decode_points) and R = 16
(2..9 points: decode_prompts on a handle with multipoint on, chunks of max_prompts / 2).  Whatever the route, a chunk is 3 tokens -> image
attentions, 2 image -> tokens attentions, 4 token segments, one upscaling launch and 4 small launches (5 with a mask prompt), and no GEMM,
LayerNorm or encoder launch.  The per-launch flops and bytes the driver books are restated below from the driver, not imported: the sums
over a call's chunks must match them exactly (all terms are integers far below 2^53)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_PROMPTS = 4
N = 5
TOKEN_SEGMENT_COLUMNS = (1280, 6016, 4992)       # S0..S2 per token row and 256-wide input; S3 depends on R: 128 + 3072 / R


def chunk_ledger(P, R, mask_input):
    """{class: (launches, flops, bytes)} of one chunk of P prompts with R token rows each"""
    nh = R // 8
    cross = 4 * (8 * R) * 4096 * 256 * P
    seg = 2 * P * R * 256
    assert 3072 % R == 0
    return {
        "decoder_t2i": (3, 3 * cross, 3 * P * 4096 * 256 * 2 * nh),
        "decoder_i2t": (2, 2 * cross, 2 * P * 4096 * 256 * 4),
        "decoder_attention": (4, seg * (sum(TOKEN_SEGMENT_COLUMNS) + 128 + 3072 // R), 0),
        "decoder_upscale": (1, 2 * P * (4096 * 256 * 256 + 16384 * 64 * 128 + 65536 * 32 * 4), P * (4096 * 256 * 2 + 4 * 65536 * 4)),
        "elementwise": (5, 0, P * (65536 * 4 + 4096 * 256 * 2)) if mask_input else (4, 0, 0),
    }


def call_ledger(n, chunk, R, mask_input):
    from saber_amd import _lib
    total = {name: [0, 0, 0] for name in _lib.PROFILE_CLASSES}
    for p0 in range(0, n, chunk):
        for name, rec in chunk_ledger(min(chunk, n - p0), R, mask_input).items():
            for i in range(3):
                total[name][i] += rec[i]
    return total


@pytest.fixture(scope="module")
def ledger_engine():
    from saber_amd.engine import Engine
    eng = Engine("tiny", seed=0, max_images=1, max_prompts=MAX_PROMPTS, precision="fp16", multipoint=True)
    g = torch.Generator(device="cpu").manual_seed(7)
    eng.encode(torch.rand(1024, 1024, generator=g).cuda())
    pts = (torch.rand(N, 2, generator=g) * 1024).cuda()
    eng.decode_points(pts, slot=0, multimask=True)          # unprofiled: builds the slot's shared src0, which is not part of a chunk's ledger
    torch.cuda.synchronize()
    mask = (torch.randn(N, 256, 256, generator=g) * 4).cuda().contiguous()
    yield eng, g, mask
    eng.close()


# (case, points per prompt (0 = decode_points), multimask, mask input, prompts per chunk, token rows)
CASES = [("a", 0, True, False, MAX_PROMPTS, 8), ("b", 0, False, True, MAX_PROMPTS, 8), ("c", 3, False, False, MAX_PROMPTS // 2, 16), ("d", 2, False, True, MAX_PROMPTS // 2, 16)]


@pytest.mark.parametrize("case,k,multimask,mask_input,chunk,R", CASES, ids=[c[0] for c in CASES])
def test_decode_ledger(ledger_engine, case, k, multimask, mask_input, chunk, R):
    eng, g, mask = ledger_engine
    mi = mask if mask_input else None
    if k == 0:
        pts = (torch.rand(N, 2, generator=g) * 1024).cuda()
        eng.profile_begin()
        outs = eng.decode_points(pts, slot=0, multimask=multimask, mask_input=mi)
    else:
        pts = (torch.rand(N, k, 2, generator=g) * 1024).cuda()
        labels = torch.ones(N, k, dtype=torch.int32).cuda()
        eng.profile_begin()
        outs = eng.decode_prompts(pts, labels, slot=0, multimask=multimask, mask_input=mi)
    prof = eng.profile_end()
    eng.check_finite()
    for t in outs:
        assert torch.isfinite(t).all()
    want = call_ledger(N, chunk, R, mask_input)
    got = {name: [rec["launches"], rec["flops"], rec["bytes"]] for name, rec in prof.items()}
    print(f"case {case}: " + "; ".join(f"{name} {rec}" for name, rec in got.items() if rec[0]))
    for name in want:
        assert got[name][0] == want[name][0], (name, "launches", got[name], want[name])
        assert got[name][1] == want[name][1], (name, "flops", got[name], want[name])
        assert got[name][2] == want[name][2], (name, "bytes", got[name], want[name])
