"""GPU tests of K8 (launch_mask_post, csrc/decoder_ops.hip) at the shapes its three kernels had never run: widths that are no multiple of
32 or 64, heights that are no multiple of the 64-row block, one-pixel and one-row crops, W > 1024 with the 64-chunk flush of very wide
rows, the idx indirection and the pass flags.  mask_post_w1k_kernel (default, W <= 1024) and mask_post_kernel<true> (debug flag 8) must be
bit-identical; mask_post_kernel<false> serves W > 1024.

Reference: fp64 bilinear upsampling (align_corners=False) of the 256 x 256 plane to the crop, source coordinate
(c + 0.5) 256 / size - 0.5 in fp64, clamped at 0, thresholded at thr, thr + offset and thr - offset.

A pixel is DECIDED for a threshold t when |v64 - t| > margin, margin = 3 2^-16 D + 8 2^-24 max|low|: D is the largest absolute difference
between adjacent low-res samples of the plane (either direction), the first term covers three fp32 roundings of a coordinate of magnitude
<= 256, the second the roundings of the two lerps.  Every decided pixel must match exactly; each count may differ from the reference count
by at most the number of undecided pixels of its threshold.  The share of undecided pixels is itself capped (max(1, 0.001 crop pixels) per
mask and threshold) and the cap is checked on the reference alone, before anything runs on the device: the margin cannot excuse a wrong kernel.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

THR, OFF = 0.0, 0.7
GUARD = 64                      # guard words before and after the bit buffer
PATTERN = 0x5a5a5a5a
INIT_STATS = (0, 0, 0, 1 << 30, 1 << 30, -1, -1, 0)      # area, inter, union, x0, y0, x1, y1, pad of a mask nothing was counted for


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_planes = {}


def planes(seed=0):
    """as tests/test_gpu_kernels.py::test_mask_post: bicubic blow-ups of 16 x 16 normal noise x 4 and one constant -5 plane (an empty mask)"""
    if seed not in _planes:
        g = torch.Generator().manual_seed(seed)
        low = F.interpolate(torch.randn(5, 1, 16, 16, generator=g) * 4, size=(256, 256), mode="bicubic")[:, 0].contiguous()
        low[4] = -5.0
        _planes[seed] = low
    return _planes[seed]


def upsample64(low, size_h, size_w):
    """fp64 bilinear, align_corners=False: [n][256][256] -> [n][size_h][size_w]"""
    def taps(size):
        s = np.maximum((np.arange(size, dtype=np.float64) + 0.5) * 256.0 / size - 0.5, 0.0)
        i0 = np.minimum(np.floor(s).astype(np.int64), 255)
        return i0, np.minimum(i0 + 1, 255), s - i0
    y0, y1, ly = taps(size_h)
    x0, x1, lx = taps(size_w)
    rows = (1.0 - ly)[None, :, None] * low[:, y0, :] + ly[None, :, None] * low[:, y1, :]
    return (1.0 - lx) * rows[:, :, x0] + lx * rows[:, :, x1]


class Reference:
    """what the fp64 upsampling decides for one set of planes and one crop"""

    def __init__(self, low, crop):
        x0, y0, cw, ch = crop
        low = low.numpy().astype(np.float64)
        self.v = upsample64(low, ch, cw)
        d = np.maximum(np.abs(np.diff(low, axis=1)).max(axis=(1, 2)), np.abs(np.diff(low, axis=2)).max(axis=(1, 2)))
        self.margin = 3 * 2.0 ** -16 * d + 8 * 2.0 ** -24 * np.abs(low).max(axis=(1, 2))
        self.cap = max(1, int(0.001 * cw * ch))
        self.above, self.undecided = {}, {}
        for name, t in (("area", THR), ("inter", THR + OFF), ("uni", THR - OFF)):
            self.above[name] = self.v > t
            self.undecided[name] = np.abs(self.v - t) <= self.margin[:, None, None]
            # a condition on the reference alone, not a measurement of the kernel
            worst = int(self.undecided[name].sum(axis=(1, 2)).max())
            assert worst <= self.cap, f"crop {crop}: {worst} undecided pixels for {name}, cap {self.cap}: choose another seed"

    def undecided_counts(self):
        return {k: u.sum(axis=(1, 2)).tolist() for k, u in self.undecided.items()}


def run(lib, low_dev, n, crop, H, W, idx=None, passf=None, ex=False, prefill=PATTERN):
    """-> (bits [n][H][W32] uint32, stats [n][8] int32); guard words around the bit buffer must come back unchanged"""
    x0, y0, cw, ch = crop
    W32 = (W + 31) // 32
    buf = torch.full((2 * GUARD + n * H * W32,), prefill, dtype=torch.int32, device="cuda")
    stats = torch.full((n, 8), 0x7b7b7b7b, dtype=torch.int32, device="cuda")
    bits_ptr = C.c_void_p(buf.data_ptr() + 4 * GUARD)
    if ex or idx is not None or passf is not None:
        st = lib.saber_k_mask_post_ex(ptr(low_dev), ptr(idx), ptr(passf), n, x0, y0, cw, ch, H, W, THR, OFF, bits_ptr, ptr(stats), None)
    else:
        st = lib.saber_k_mask_post(ptr(low_dev), n, x0, y0, cw, ch, H, W, THR, OFF, bits_ptr, ptr(stats), None)
    assert st == 0, lib.saber_k_last_error().decode()
    torch.cuda.synchronize()
    buf = buf.cpu().numpy().view(np.uint32)
    assert (buf[:GUARD] == prefill).all() and (buf[-GUARD:] == prefill).all(), "a word outside the bit buffer was written"
    return buf[GUARD:-GUARD].reshape(n, H, W32).copy(), stats.cpu().numpy()


def unpack(bits):
    """[n][H][W32] uint32 -> [n][H][32 W32] bool, bit b of word w = pixel 32 w + b"""
    n, H, W32 = bits.shape
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(n, H, W32 * 4), axis=-1, bitorder="little").astype(bool)


def check(ref, bits, stats, crop, H, W, masks=None):
    """bits / stats of the kernel for the planes `masks` of the reference (default: all, in order)"""
    x0, y0, cw, ch = crop
    masks = list(range(ref.v.shape[0])) if masks is None else masks
    got = unpack(bits)
    assert not got[:, :, W:].any(), "bits at columns >= W"
    got = got[:, :, :W]
    outside = np.ones((H, W), bool)
    outside[y0:y0 + ch, x0:x0 + cw] = False
    assert not got[:, outside].any(), "bits outside the crop"
    rows_out = np.ones(H, bool)
    rows_out[y0:y0 + ch] = False
    assert not bits[:, rows_out].any(), "words of rows outside the crop are zero"
    for i, m in enumerate(masks):
        g = got[i, y0:y0 + ch, x0:x0 + cw]
        und = ref.undecided["area"][m]
        wrong = (g != ref.above["area"][m]) & ~und
        assert not wrong.any(), (i, m, int(wrong.sum()), "decided pixels differ")
        area, inter, uni = (int(v) for v in stats[i, :3])
        assert area == int(g.sum()), (i, area, int(g.sum()))                      # area is the popcount of the returned bits
        for name, val in (("area", area), ("inter", inter), ("uni", uni)):
            want, slack = int(ref.above[name][m].sum()), int(ref.undecided[name][m].sum())
            assert abs(val - want) <= slack, (i, m, name, val, want, slack)
        if area:
            ys, xs = np.where(got[i])
            assert tuple(stats[i, 3:7]) == (xs.min(), ys.min(), xs.max(), ys.max()), (i, stats[i])
        else:
            assert tuple(stats[i]) == INIT_STATS, (i, stats[i])
        if m == 4:
            assert area == 0                                                      # the constant -5 plane is an empty mask


def crops_of(H, W):
    return {"full": (0, 0, W, H),
            "interior": (W // 7 + 1, H // 5 + 2, W - W // 7 - W // 3 - 2, H - H // 5 - H // 4 - 3),     # ragged, touches no edge
            "flush": (W - (2 * W // 3 + 1), H - (H // 2 + 3), 2 * W // 3 + 1, H // 2 + 3),             # right and bottom edges
            "pixel": (W - W // 3, H // 2 + 1, 1, 1),
            "row": (W // 9, H - H // 3, W - W // 9 - 5, 1)}


SMALL = [(100, 75), (70, 130), (200, 1000), (65, 1024), (129, 96)]
WIDE = {(40, 1100): [(900, 5, 170, 30), (0, 0, 1100, 40)],                  # 35 words per row; the interior crop straddles column 1024
        (20, 4160): [(1000, 3, 3130, 14), (0, 0, 4160, 20)]}                # crosses the 64-chunk flush; straddles columns 1024 and 4096


@pytest.fixture(scope="module")
def low_dev(gpu_lib):
    return planes().cuda()


@pytest.mark.parametrize("which", ["full", "interior", "flush", "pixel", "row"])
@pytest.mark.parametrize("H,W", SMALL)
def test_mask_post_small_shapes(gpu_lib, low_dev, H, W, which):
    crop = crops_of(H, W)[which]
    x0, y0, cw, ch = crop
    assert x0 >= 0 and y0 >= 0 and cw >= 1 and ch >= 1 and x0 + cw <= W and y0 + ch <= H
    ref = Reference(planes(), crop)                     # asserts the cap on undecided pixels before the device runs
    print(f"mask_post {H}x{W} {which} {crop}: undecided {ref.undecided_counts()} cap {ref.cap}")
    bits, stats = run(gpu_lib, low_dev, 5, crop, H, W)                  # mask_post_w1k_kernel
    try:
        gpu_lib.saber_k_set_debug(8)
        bits8, stats8 = run(gpu_lib, low_dev, 5, crop, H, W)            # mask_post_kernel<true>
    finally:
        gpu_lib.saber_k_set_debug(0)
    check(ref, bits, stats, crop, H, W)
    check(ref, bits8, stats8, crop, H, W)
    assert np.array_equal(bits, bits8) and np.array_equal(stats, stats8), "the two W <= 1024 kernels disagree"


@pytest.mark.parametrize("H,W,k", [(H, W, k) for (H, W), cs in WIDE.items() for k in range(len(cs))])
def test_mask_post_wide_shapes(gpu_lib, low_dev, H, W, k):
    crop = WIDE[(H, W)][k]
    ref = Reference(planes(), crop)
    print(f"mask_post {H}x{W} {crop}: undecided {ref.undecided_counts()} cap {ref.cap}")
    bits, stats = run(gpu_lib, low_dev, 5, crop, H, W)                  # mask_post_kernel<false>
    check(ref, bits, stats, crop, H, W)


@pytest.mark.parametrize("H,W,crop,flag", [(70, 130, (19, 16, 68, 37), 0), (70, 130, (19, 16, 68, 37), 8), (40, 1100, (900, 5, 170, 30), 0)])
def test_mask_post_ex_idx_and_pass(gpu_lib, low_dev, H, W, crop, flag):
    """idx: mask i reads plane idx[i]; pass: masks with 0 keep their bits and the initial statistics"""
    order = [4, 0, 2]
    ref = Reference(planes(), crop)
    idx = torch.tensor(order, dtype=torch.int32).cuda()
    direct_dev = planes()[order].contiguous().cuda()
    try:
        gpu_lib.saber_k_set_debug(flag)
        direct = run(gpu_lib, direct_dev, 3, crop, H, W)
        via_idx = run(gpu_lib, low_dev, 3, crop, H, W, idx=idx)
        null_ex = run(gpu_lib, direct_dev, 3, crop, H, W, ex=True)                  # both pointers null: saber_k_mask_post
        passf = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
        skipped = run(gpu_lib, low_dev, 3, crop, H, W, idx=idx, passf=passf, prefill=0x3c3c3c3c)
    finally:
        gpu_lib.saber_k_set_debug(0)
    check(ref, *direct, crop, H, W, masks=order)
    for other in (via_idx, null_ex):
        assert np.array_equal(direct[0], other[0]) and np.array_equal(direct[1], other[1])
    bits, stats = skipped
    assert (bits[1] == 0x3c3c3c3c).all(), "the bits of a skipped mask were written"
    assert tuple(stats[1]) == INIT_STATS
    for i in (0, 2):
        assert np.array_equal(bits[i], direct[0][i]) and np.array_equal(stats[i], direct[1][i])
