"""GPU tests of the kernels at the entry of the image path, called directly through the kernel-level C-ABI and compared with fp64:

  K1a resize_normalize_kernel (saber_k_resize_normalize)  against a numpy restatement of ATen's antialiased bilinear tap rule
  K1b patch_embed_kernel      (saber_k_patch_embed)       against an fp64 convolution (k 7, stride 4, zero padding 3) + bias + pos
  K0  saber_k_prepare at ragged / non-square shapes, sides below the 500-wide filter and at the LDS side limit, against the scipy oracle

Resize reference.  lo, n, centre and 1 / scale of every output index come from the fp32 expressions of axis_taps (csrc/image_ops.hip), the
triangle weights of those taps, their normalisation, the horizontal-then-vertical sums and (v - mean) / std are fp64.  The restatement is
pinned to torch's fp64 F.interpolate(mode="bilinear", antialias=True, align_corners=False) on the same crops (2e-6), not to the kernel.

Resize bound.  Before normalisation an output is a convex combination of inputs in [0, 1]: the fp32 chain of n_x horizontal and n_y vertical
multiply-adds costs at most (n_x + n_y) 2^-24, the two weight normalisations and the final subtract and divide at most 8 more; that error is
divided by std_c.  The bound is evaluated per output from the reference's own tap counts.

Patch-embedding bound.  A 147-term fp32 fma chain plus two adds: 150 2^-24 (sum |v w| + |bias| + |pos|) per output, evaluated in fp64.

Measured (largest error / bound): resize grey crops 0.21, RGB down-scale 0.26, channels -1 0.20 (restatement against ATen fp64: 2.8e-8);
patch embedding 0.036 / 0.038 / 0.041 for C = 96 / 112 / 144; prepare <= 1.6e-6 (u16) and 1.8e-7 (f32) against its 2e-4.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
MEAN = np.array([0.485, 0.456, 0.406], np.float32)      # the kernel's fp32 constants
STD = np.array([0.229, 0.224, 0.225], np.float32)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def kcall(lib, st):
    assert st == 0, lib.saber_k_last_error().decode()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ K1a
def axis_weights(in_size, out_size):
    """(weights [out_size][in_size] fp64, rows sum to 1; tap count per output index).  lo, n, centre, 1 / scale: fp32, as axis_taps"""
    f = np.float32
    o = np.arange(out_size, dtype=np.float32)
    scale = f(in_size) / f(out_size)
    support = scale if scale >= f(1) else f(1)
    inv = f(1) / scale if scale >= f(1) else f(1)
    center = scale * (o + f(0.5))
    assert scale.dtype == np.float32 and center.dtype == np.float32 and np.asarray(inv).dtype == np.float32
    lo = np.maximum((center - support + f(0.5)).astype(np.int32), 0)
    n = np.minimum((center + support + f(0.5)).astype(np.int32), in_size) - lo
    assert (n >= 1).all()
    j = np.arange(in_size)[None, :]
    x = np.abs((j - center.astype(np.float64)[:, None] + 0.5) * float(inv))
    w = np.where(x < 1.0, 1.0 - x, 0.0)
    w[(j < lo[:, None]) | (j >= (lo + n)[:, None])] = 0.0
    return w / w.sum(1, keepdims=True), n


def resize_ref(img, crop, res):
    """img (H,W) or (H,W,3) -> (fp64 [C][res][res] before normalisation, n_x [res], n_y [res])"""
    x0, y0, x1, y1 = crop
    c = img[y0:y1, x0:x1].astype(np.float64)
    c = c[None] if c.ndim == 2 else c.transpose(2, 0, 1)
    wx, nx = axis_weights(x1 - x0, res)
    wy, ny = axis_weights(y1 - y0, res)
    return np.einsum("oy,cyx->cox", wy, c @ wx.T), nx, ny      # horizontally first, then vertically


def aten_ref(img, crop, res):
    x0, y0, x1, y1 = crop
    c = torch.from_numpy(img[y0:y1, x0:x1].astype(np.float64))
    c = c[None] if c.dim() == 2 else c.permute(2, 0, 1)
    return F.interpolate(c[None], size=(res, res), mode="bilinear", antialias=True, align_corners=False)[0].numpy()


def run_resize(lib, img_dev, H, W, channels, crops, res, expect=0):
    n = len(crops)
    crops_dev = torch.tensor(crops, dtype=torch.int32).cuda()
    out = torch.full((n, 3, res, res), -77.0, device="cuda")
    st = lib.saber_k_resize_normalize(ptr(img_dev), H, W, channels, ptr(crops_dev), n, ptr(out), res, None)
    torch.cuda.synchronize()
    assert st == expect, lib.saber_k_last_error().decode()
    return out.cpu().numpy()


GREY_HW = (80, 112)
GREY_CROPS = [(0, 0, 112, 80),          # the full image
              (0, 0, 64, 64),           # identity scale at the origin
              (48, 16, 112, 80),        # identity scale flush with the bottom-right corner
              (31, 22, 84, 59),         # 53 x 37 interior: ragged up-scale
              (70, 41, 71, 42),         # 1 x 1
              (0, 50, 112, 53)]         # 112 x 3: down in x, up in y
RGB_HW = (850, 1150)
RGB_CROPS = [(0, 0, 1150, 850),         # the full image: tens of taps per axis
             (301, 222, 898, 622),      # 597 x 400 interior
             (1020, 785, 1150, 850)]    # 130 x 65 flush with the bottom-right corner
RES = 64


class ResizeCase:
    def __init__(self, name, hw, channels, crops, seed):
        rng = np.random.default_rng(seed)
        self.name, self.hw, self.channels, self.crops = name, hw, channels, crops
        self.img = rng.uniform(0.0, 1.0, hw + ((3,) if channels == 3 else ())).astype(np.float32)
        self.ref = [resize_ref(self.img, c, RES) for c in crops]
        for c, (r, _, _) in zip(crops, self.ref):                   # the reference is pinned to ATen, not to the kernel
            d = np.abs(r - aten_ref(self.img, c, RES)).max()
            print(f"resize reference vs ATen fp64, {name} crop {c}: max |diff| {d:.2e}")
            assert d <= 2e-6, (name, c, d)

    def check(self, out, normalised=True, label=""):
        """out [n][3][RES][RES] of the kernel against the reference; prints and returns the largest ratio of error to bound"""
        worst = 0.0
        for b, (r, nx, ny) in enumerate(self.ref):
            taps = (nx[None, :] + ny[:, None] + 8) * U24
            for c in range(3):
                want = r[c if self.channels == 3 else 0]
                bound = taps
                if normalised:
                    want = (want - float(MEAN[c])) / float(STD[c])
                    bound = taps / float(STD[c])
                ratio = (np.abs(out[b, c].astype(np.float64) - want) / bound).max()
                worst = max(worst, ratio)
                assert ratio <= 1.0, (self.name, self.crops[b], c, ratio)
            print(f"resize_normalize {self.name}{label} crop {self.crops[b]}: taps x {nx.min()}..{nx.max()} y {ny.min()}..{ny.max()}")
        print(f"resize_normalize {self.name}{label}: largest error / bound {worst:.3f}")
        return worst


@pytest.fixture(scope="module")
def grey_case():
    return ResizeCase("grey 80x112", GREY_HW, 1, GREY_CROPS, 11)


@pytest.fixture(scope="module")
def rgb_case():
    return ResizeCase("rgb 850x1150", RGB_HW, 3, RGB_CROPS, 12)


def test_resize_grey_crops(gpu_lib, grey_case):
    """one launch, six crops of different sizes (blockIdx.z and the per-crop table): identity, ragged up-scale, 1 x 1, mixed down / up"""
    k = grey_case
    out = run_resize(gpu_lib, torch.from_numpy(k.img).cuda(), *k.hw, 1, k.crops, RES)
    k.check(out)


def test_resize_rgb_downscale(gpu_lib, rgb_case):
    """antialiased down-scale of an image larger than the model input (up to 37 taps per axis), interleaved RGB"""
    k = rgb_case
    out = run_resize(gpu_lib, torch.from_numpy(k.img).cuda(), *k.hw, 3, k.crops, RES)
    k.check(out)


def test_resize_grey_without_statistics(gpu_lib, grey_case):
    """channels = -1: the un-normalised resize, replicated into three planes"""
    k = grey_case
    out = run_resize(gpu_lib, torch.from_numpy(k.img).cuda(), *k.hw, -1, k.crops, RES)
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 0], out[:, 2])
    k.check(out, normalised=False, label=" channels -1")
    # the same convex combination as channels = 1 before its subtract and divide
    norm = run_resize(gpu_lib, torch.from_numpy(k.img).cuda(), *k.hw, 1, k.crops, RES)
    for c in range(3):
        assert np.array_equal(((out[:, c] - MEAN[c]) / STD[c]).astype(np.float32), norm[:, c]), c


def test_resize_identity_1024_is_bitwise(gpu_lib):
    """scale 1: one tap of weight 1 per axis, so the output is (v - mean_c) / std_c evaluated in float32, bit for bit"""
    img = np.random.default_rng(13).uniform(0.0, 1.0, (1024, 1024)).astype(np.float32)
    out = run_resize(gpu_lib, torch.from_numpy(img).cuda(), 1024, 1024, 1, [(0, 0, 1024, 1024)], 1024)
    for c in range(3):
        want = (img - MEAN[c]) / STD[c]
        assert want.dtype == np.float32
        assert np.array_equal(out[0, c].view(np.uint32), want.view(np.uint32)), c


@pytest.mark.parametrize("which", ["grey", "rgb"])
def test_resize_reads_the_crop_only(gpu_lib, grey_case, rgb_case, which):
    """ATen resizes the cropped tensor: taps clamp at the crop's edges, not the image's.  With every pixel outside a crop set to NaN the
    crop's output must not change by a bit."""
    k = grey_case if which == "grey" else rgb_case
    base = run_resize(gpu_lib, torch.from_numpy(k.img).cuda(), *k.hw, k.channels, k.crops, RES)
    assert np.isfinite(base).all()
    for b, (x0, y0, x1, y1) in enumerate(k.crops):
        img = np.full_like(k.img, np.nan)
        img[y0:y1, x0:x1] = k.img[y0:y1, x0:x1]
        out = run_resize(gpu_lib, torch.from_numpy(img).cuda(), *k.hw, k.channels, [k.crops[b]], RES)
        assert np.array_equal(out[0].view(np.uint32), base[b].view(np.uint32)), k.crops[b]


def test_resize_refuses_res_that_is_no_multiple_of_16(gpu_lib, grey_case):
    """the launcher's grid is res / 16 blocks per axis: res = 40 would leave a border of 8 unwritten, so the entry point refuses it"""
    k = grey_case
    img_dev = torch.from_numpy(k.img).cuda()
    crops_dev = torch.tensor(k.crops[:1], dtype=torch.int32).cuda()
    out = torch.full((1, 3, 48, 48), -77.0, device="cuda")
    for res in (40, 0, -16):
        assert gpu_lib.saber_k_resize_normalize(ptr(img_dev), *k.hw, 1, ptr(crops_dev), 1, ptr(out), res, None) == -1
        assert b"multiple of 16" in gpu_lib.saber_k_last_error()
    torch.cuda.synchronize()
    assert (out == -77.0).all()                        # nothing was launched
    assert (run_resize(gpu_lib, img_dev, *k.hw, 1, k.crops[:1], 48) != -77.0).all()      # 48 is accepted and fills the output


# ------------------------------------------------------------------------------------------------ K1b
@pytest.fixture(scope="module")
def embed_input(gpu_lib):
    """pix [2][3][1024][1024], its 7 x 7 stride-4 patches in fp64 [2][65536][147] (tap = (c 7 + ky) 7 + kx, zero padding 3) and the engine's
    token row of every (y, x) of the 256 x 256 grid"""
    g = torch.Generator().manual_seed(21)
    pix = torch.randn(2, 3, 1024, 1024, generator=g).cuda()
    pad = F.pad(pix.double(), (3, 3, 3, 3))
    cols = torch.stack([pad[:, c, ky:ky + 1021:4, kx:kx + 1021:4] for c in range(3) for ky in range(7) for kx in range(7)], dim=-1)
    rows = np.array([[gpu_lib.saber_k_perm_index(y, x, 0) for x in range(256)] for y in range(256)]).ravel()
    assert sorted(rows.tolist()) == list(range(65536))
    yield pix, cols.reshape(2, 65536, 147), torch.from_numpy(rows).cuda()
    del pix, pad, cols
    torch.cuda.empty_cache()


@pytest.mark.parametrize("Cdim", [96, 112, 144])
def test_patch_embed(gpu_lib, embed_input, Cdim):
    """all 65536 x C outputs of both images (the 65536-row image stride; the image-border tokens read padding)"""
    pix, cols, rows = embed_input
    g = torch.Generator().manual_seed(Cdim)
    wt = (torch.randn(147, Cdim, generator=g) / 147 ** 0.5).cuda()
    bias = torch.randn(Cdim, generator=g).cuda()
    pos = torch.randn(65536, Cdim, generator=g).cuda()
    out = torch.full((2, 65536, Cdim), float("nan"), device="cuda")
    kcall(gpu_lib, gpu_lib.saber_k_patch_embed(ptr(pix), ptr(wt), ptr(bias), ptr(pos), ptr(out), 2, Cdim, None))
    ref = torch.empty(2, 65536, Cdim, dtype=torch.float64, device="cuda")
    mag = torch.empty_like(ref)
    ref[:, rows] = cols @ wt.double() + bias.double()
    mag[:, rows] = cols.abs() @ wt.double().abs() + bias.double().abs()
    ref += pos.double()
    mag += pos.double().abs()
    ratio = ((out.double() - ref).abs() / (150 * U24 * mag)).max().item()
    print(f"patch_embed C={Cdim}: largest error / bound {ratio:.3f}")
    assert ratio <= 1.0            # NaN (an output the kernel did not write) fails too
    assert torch.isfinite(out).all()


def test_patch_embed_refuses_an_unsupported_width(gpu_lib, embed_input):
    pix = embed_input[0]
    wt, bias, pos = torch.zeros(147, 128).cuda(), torch.zeros(128).cuda(), torch.zeros(65536, 128).cuda()
    out = torch.full((2, 65536, 128), -77.0, device="cuda")
    assert gpu_lib.saber_k_patch_embed(ptr(pix), ptr(wt), ptr(bias), ptr(pos), ptr(out), 2, 128, None) == -1
    assert b"unsupported embed dim" in gpu_lib.saber_k_last_error()
    torch.cuda.synchronize()
    assert (out == -77.0).all()


# ------------------------------------------------------------------------------------------------ K0
def prepare_input(H, W, dtype, seed):
    """a noisy slice with an illumination ramp, as uint16 counts or as the float32 values of tests/test_gpu_kernels.py::test_prepare"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    img = rng.normal(32768.0, 3000.0, (H, W)) + 4000.0 * (xx / W - 0.5) + 2500.0 * np.sin((yy + 0.5) / H * np.pi)
    img = np.clip(np.rint(img), 0, 65535).astype(np.uint16)
    return img if dtype == "u16" else ((img.astype(np.float32) - 30000.0) / 7.0)


def run_prepare(lib, img, expect=0):
    H, W = img.shape
    dev = torch.from_numpy(img).cuda()
    out = torch.full((H, W), -77.0, device="cuda")
    ws = torch.zeros(4, H, W, device="cuda")
    mm = torch.full((2,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    st = lib.saber_k_prepare(ptr(dev), 0 if img.dtype == np.uint16 else 1, H, W, ptr(out), ptr(ws), ptr(mm), None)
    torch.cuda.synchronize()
    assert st == expect, lib.saber_k_last_error().decode()
    return out.cpu().numpy(), mm.cpu().numpy()


def check_prepare(out, ref, what):
    err = np.abs(out - ref).max()
    print(f"prepare {what}: max |diff| {err:.2e}")
    assert err < 2e-4, (what, err)
    assert out.min() == 0.0 and abs(float(out.max()) - 1.0) < 1e-6


@pytest.mark.parametrize("H,W,dtype", [(37, 53, "u16"), (37, 53, "f32"), (250, 251, "u16"), (250, 251, "f32"), (499, 500, "u16"), (499, 500, "f32"),
                                       (501, 130, "f32"), (96, 1300, "f32"), (1, 64, "f32")])
def test_prepare_ragged_shapes(gpu_lib, H, W, dtype):
    """non-square and odd sides; sides far below half the 500-wide filter wrap the reflect extension several times"""
    from oracle import saber_ref
    img = prepare_input(H, W, dtype, H * 7 + W)
    out, _ = run_prepare(gpu_lib, img)
    check_prepare(out, saber_ref.prepare(img.astype(np.float32)), f"{H}x{W} {dtype}")


def test_prepare_small_rgb(gpu_lib):
    """(H,W,3) far below the filter size, through the reference-signature wrapper"""
    from oracle import saber_ref
    from saber_amd.utils import preprocessing as prep
    rgb = np.random.default_rng(5).uniform(0.0, 1.0, (45, 70, 3)).astype(np.float32)
    out = prep.prepare(rgb, to_rgb=False)
    assert out.shape == rgb.shape and out.dtype == torch.float32
    err = np.abs(out.cpu().numpy() - saber_ref.prepare(rgb)).max()
    print(f"prepare rgb 45x70x3: max |diff| {err:.2e}")
    assert err < 2e-4


def largest_prepare_side():
    """the largest side prepare_impl (csrc/image_ops.hip) accepts, from its own lds_bytes formula: two double lines of npad + 1 entries,
    npad = the reflect-extended length L + 499 rounded up to 256, within 152 KiB"""
    def lds_bytes(L, size=500):
        npad = (L + size - 1 + 255) // 256 * 256
        return 2 * (npad + 1) * 8
    L = 1
    while lds_bytes(L + 1) <= 152 * 1024:
        L += 1
    assert lds_bytes(L) <= 152 * 1024 < lds_bytes(L + 1)
    return L


def test_prepare_side_limit(gpu_lib):
    from oracle import saber_ref
    L = largest_prepare_side()
    print(f"prepare: largest accepted side {L}")
    img = prepare_input(16, L + 1, "f32", 3)
    out, mm = run_prepare(gpu_lib, img, expect=-1)                      # one column too wide: refused, nothing launched
    assert b"too large for the LDS line buffer" in gpu_lib.saber_k_last_error()
    assert (out == -77.0).all() and (mm == 0x5a5a5a5a).all()
    out, mm = run_prepare(gpu_lib, np.ascontiguousarray(img.T), expect=-1)   # the same for the other axis
    assert (out == -77.0).all() and (mm == 0x5a5a5a5a).all()
    img = np.ascontiguousarray(img[:, :L])
    out, _ = run_prepare(gpu_lib, img)                                  # exactly at the limit: runs
    check_prepare(out, saber_ref.prepare(img), f"16x{L} f32")
