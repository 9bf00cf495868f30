"""GPU tests of K8's full-line store path and of its group launch (mask_post_w1k_kernel<WIDE>, launch_mask_post_group; csrc/decoder_ops.hip).

The default W <= 1024 kernel collects the 16 rows of a wave in LDS and writes them as 16 bytes per lane when a row of bits is a whole
number of 16-byte pieces at a 16-byte aligned address (W32 % 4 == 0), keeps one narrow store pair per row otherwise, zero-fills waves and
workgroups the crop does not touch without any set-up, and takes its horizontal taps from a table the workgroup computes once.  None of
that may change a bit: in every case here the default path must equal mask_post_kernel<true> (debug flag 8, the reference path) in the
bits and in all seven statistics, the words of a skipped mask must keep their pattern, and the guard words around the buffer must be intact.
The fp64 comparison of both kernels is tests/test_gpu_mask_post_shapes.py's.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

THR, OFF = 0.0, 0.7
GUARD = 64                      # guard words before and after the bit buffer (64 words keep the bits 16-byte aligned, 65 do not)
PATTERN = 0x5a5a5a5a
INIT_STATS = (0, 0, 0, 1 << 30, 1 << 30, -1, -1, 0)      # area, inter, union, x0, y0, x1, y1, pad of a mask nothing was counted for


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_planes = {}


def planes(seed=0):
    """the recipe of tests/test_gpu_mask_post_shapes.py: bicubic blow-ups of 16 x 16 normal noise x 4 and one constant -5 plane (an empty mask)"""
    if seed not in _planes:
        g = torch.Generator().manual_seed(seed)
        low = F.interpolate(torch.randn(5, 1, 16, 16, generator=g) * 4, size=(256, 256), mode="bicubic")[:, 0].contiguous()
        low[4] = -5.0
        _planes[seed] = low
    return _planes[seed]


@pytest.fixture(scope="module")
def low_dev(gpu_lib):
    return planes().cuda()


def launch(lib, n, H, W, call, guard=GUARD, prefill=PATTERN):
    """call(bits_ptr, stats) launches K8 for n masks -> (bits [n][H][W32] uint32, stats [n][8] int32); checks the guard words"""
    W32 = (W + 31) // 32
    buf = torch.full((2 * guard + n * H * W32,), prefill, dtype=torch.int32, device="cuda")
    stats = torch.full((n, 8), 0x7b7b7b7b, dtype=torch.int32, device="cuda")
    call(buf.data_ptr() + 4 * guard, stats)
    torch.cuda.synchronize()
    buf = buf.cpu().numpy().view(np.uint32)
    assert (buf[:guard] == prefill).all() and (buf[-guard:] == prefill).all(), "a word outside the bit buffer was written"
    return buf[guard:-guard].reshape(n, H, W32).copy(), stats.cpu().numpy()


def run_ex(lib, low_dev, n, crop, H, W, idx=None, passf=None, **kw):
    x0, y0, cw, ch = crop

    def call(bits_addr, stats):
        st = lib.saber_k_mask_post_ex(ptr(low_dev), ptr(idx), ptr(passf), n, x0, y0, cw, ch, H, W, THR, OFF, C.c_void_p(bits_addr), ptr(stats), None)
        assert st == 0, lib.saber_k_last_error().decode()
    return launch(lib, n, H, W, call, **kw)


def both(lib, fn):
    """fn() on the default path and on the reference path (debug flag 8)"""
    got = fn()
    try:
        lib.saber_k_set_debug(8)
        want = fn()
    finally:
        lib.saber_k_set_debug(0)
    return got, want


def assert_same(got, want):
    assert np.array_equal(got[1], want[1]), ("statistics differ", got[1], want[1])
    diff = np.argwhere(got[0] != want[0])
    assert diff.size == 0, (f"{len(diff)} words differ, the first (mask, row, word)", diff[0])


def unpack(bits):
    n, H, W32 = bits.shape
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(n, H, W32 * 4), axis=-1, bitorder="little").astype(bool)


def check_inside(bits, stats, crop, nonempty):
    """sanity on top of the equality: no bit outside the crop, area = popcount, the box is that of the bits"""
    x0, y0, cw, ch = crop
    got = unpack(bits)
    outside = np.ones(got.shape[1:], bool)
    outside[y0:y0 + ch, x0:x0 + cw] = False
    assert not got[:, outside].any(), "bits outside the crop"
    for i in range(bits.shape[0]):
        assert int(stats[i, 0]) == int(got[i].sum())
        if stats[i, 0]:
            ys, xs = np.where(got[i])
            assert tuple(stats[i, 3:7]) == (xs.min(), ys.min(), xs.max(), ys.max())
        else:
            assert tuple(stats[i]) == INIT_STATS
    if nonempty:
        assert stats[:, 0].max() > 0, "the case counts nothing: it would prove nothing"


CASES_1K = {"interior362": (331, 331, 362, 362),        # starts and ends inside a 16-row group and inside a 64-pixel chunk
            "full": (0, 0, 1024, 1024),
            "row15": (0, 15, 1024, 1), "row16": (0, 16, 1024, 1),          # last row of a wave's group / first row of the next
            "col63": (63, 0, 1, 1024), "col64": (64, 0, 1, 1024)}          # last pixel of a chunk / first pixel of the next


@pytest.mark.parametrize("which", list(CASES_1K))
def test_wide_1024(gpu_lib, low_dev, which):
    crop = CASES_1K[which]
    got, want = both(gpu_lib, lambda: run_ex(gpu_lib, low_dev, 5, crop, 1024, 1024))
    assert_same(got, want)
    check_inside(*got, crop, nonempty=True)


@pytest.mark.parametrize("H,W,crop,guard", [(1000, 992, (40, 123, 700, 650), GUARD),       # rows of 124 bytes: no 16-byte pieces
                                            (1000, 992, (0, 0, 992, 1000), GUARD),
                                            (17, 40, (3, 2, 30, 14), GUARD),                # two words per row, one ragged workgroup
                                            (17, 40, (0, 0, 40, 17), GUARD),
                                            (1000, 1024, (331, 600, 362, 400), GUARD),      # wide rows, H no multiple of 16: the last wave holds 8 rows
                                            (72, 250, (100, 10, 120, 60), GUARD),           # 8 words per row: 32-byte rows through the wide path
                                            (1024, 1024, (331, 331, 362, 362), GUARD + 1)])  # bits 4 bytes off a 16-byte boundary
def test_other_widths_and_alignment(gpu_lib, low_dev, H, W, crop, guard):
    n = 3 if H * W > 500000 else 5
    got, want = both(gpu_lib, lambda: run_ex(gpu_lib, low_dev, n, crop, H, W, guard=guard))
    assert_same(got, want)
    check_inside(*got, crop, nonempty=True)


@pytest.mark.parametrize("H,W,crop", [(1024, 1024, (331, 331, 362, 362)), (1000, 992, (40, 123, 700, 650))])
def test_pass_and_idx(gpu_lib, low_dev, H, W, crop):
    """pass = [1, 0, 1] with idx a permutation: the skipped mask's words keep their pattern and its statistics are the initial record"""
    idx = torch.tensor([3, 0, 2], dtype=torch.int32).cuda()
    passf = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
    got, want = both(gpu_lib, lambda: run_ex(gpu_lib, low_dev, 3, crop, H, W, idx=idx, passf=passf, prefill=0x3c3c3c3c))
    assert_same(got, want)
    bits, stats = got
    assert (bits[1] == 0x3c3c3c3c).all(), "the words of a skipped mask were written"
    assert tuple(stats[1]) == INIT_STATS
    direct = run_ex(gpu_lib, planes()[[3, 0, 2]].contiguous().cuda(), 3, crop, H, W)
    for i in (0, 2):
        assert np.array_equal(bits[i], direct[0][i]) and np.array_equal(stats[i], direct[1][i])
    assert stats[0, 0] > 0 and stats[2, 0] > 0


def crop_table(crops, counts, kbase0):
    """[n][8] int32: x0, y0, x1, y1, kbase, nm, two words K8 does not read"""
    rows, k = [], kbase0
    for (x0, y0, cw, ch), nm in zip(crops, counts):
        rows.append([x0, y0, x0 + cw, y0 + ch, k, nm, -1, -1])
        k += nm
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("H,W", [(1024, 1024), (200, 1000)])
@pytest.mark.parametrize("with_pass", [False, True])
def test_group_launch(gpu_lib, low_dev, H, W, with_pass):
    """two crops of different size and position in one saber_k_mask_post_group call = one saber_k_mask_post_ex call per crop"""
    crops = [(331, 331, 362, 362), (427, 0, 597, 597)] if H == 1024 else [(70, 33, 501, 90), (3, 100, 300, 100)]
    counts = [3, 2]
    idx = torch.tensor([4, 1, 0, 2, 3], dtype=torch.int32).cuda()
    passf = torch.tensor([1, 0, 1, 0, 1], dtype=torch.uint8).cuda() if with_pass else None
    table = crop_table(crops, counts, kbase0=7)
    table_dev = table.cuda()
    W32 = (W + 31) // 32

    def group_call(bits_addr, stats):
        st = gpu_lib.saber_k_mask_post_group(ptr(low_dev), ptr(idx), ptr(passf), ptr(table), ptr(table_dev), 2, H, W, THR, OFF, C.c_void_p(bits_addr), ptr(stats), None)
        assert st == 0, gpu_lib.saber_k_last_error().decode()

    def per_crop_call(bits_addr, stats):
        off = 0
        for (x0, y0, cw, ch), nm in zip(crops, counts):
            st = gpu_lib.saber_k_mask_post_ex(ptr(low_dev), C.c_void_p(idx.data_ptr() + 4 * off), None if passf is None else C.c_void_p(passf.data_ptr() + off), nm,
                                              x0, y0, cw, ch, H, W, THR, OFF, C.c_void_p(bits_addr + 4 * off * H * W32), C.c_void_p(stats.data_ptr() + 32 * off), None)
            assert st == 0, gpu_lib.saber_k_last_error().decode()
            off += nm

    got = launch(gpu_lib, 5, H, W, group_call, prefill=0x3c3c3c3c)
    want_default = launch(gpu_lib, 5, H, W, per_crop_call, prefill=0x3c3c3c3c)
    try:
        gpu_lib.saber_k_set_debug(8)
        want_ref = launch(gpu_lib, 5, H, W, per_crop_call, prefill=0x3c3c3c3c)
        got_ref = launch(gpu_lib, 5, H, W, group_call, prefill=0x3c3c3c3c)       # the group entry point on the reference path: crop by crop
    finally:
        gpu_lib.saber_k_set_debug(0)
    for other in (want_default, want_ref, got_ref):
        assert_same(got, other)
    bits, stats = got
    for i in range(5):
        if with_pass and i in (1, 3):
            assert (bits[i] == 0x3c3c3c3c).all() and tuple(stats[i]) == INIT_STATS, "a skipped mask was touched"
    check_inside(bits[[0, 2]], stats[[0, 2]], crops[0], nonempty=False)
    check_inside(bits[[4]], stats[[4]], crops[1], nonempty=True)


def test_group_launch_rejects_gaps(gpu_lib, low_dev):
    table = torch.tensor([[0, 0, 64, 64, 0, 2, 0, 0], [0, 0, 64, 64, 3, 2, 0, 0]], dtype=torch.int32)      # candidate 2 belongs to no crop
    bits = torch.zeros(5 * 64 * 2, dtype=torch.int32, device="cuda")
    stats = torch.zeros(5, 8, dtype=torch.int32, device="cuda")
    st = gpu_lib.saber_k_mask_post_group(ptr(low_dev), None, None, ptr(table), ptr(table.cuda()), 2, 64, 64, THR, OFF, ptr(bits), ptr(stats), None)
    assert st != 0 and b"consecutive" in gpu_lib.saber_k_last_error()
    torch.cuda.synchronize()
    assert not bits.any().item()
