"""GPU: slab preparation on the device (csrc/volprep.hip, saber_amd/utils/volprep.py): the z Gaussian with fused min / max, the min-max
normalisation and the slab projection of tomoSegmenter.segment_vol (reference saber/segmenters/tomo.py:98-101), the kernels through the
C-ABI and the tensor routes of the public functions built on them.

The smoothing is checked against scipy.ndimage.correlate1d in float64 (input and the fp32 taps widened) with the bound of a ks-term fp32
dot product, B = (ks + 1) 2^-24 sum_k |w_k| |x|, at every voxel; everything else is checked bit for bit against numpy on the host copy."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, I16, U16, U8 = 0, 1, 2, 3


def _taps(sigma):
    from saber_amd.utils.volprep import make_gaussian_kernel
    return make_gaussian_kernel(sigma)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _to_dev(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _correlate(lib, x_dev, dtype, w, dim, chunk_len=0, minmax=True):
    """saber_k_correlate1d_zero on a contiguous device array; returns (out, minmax) and checks that the input kept its bits"""
    shape = tuple(x_dev.shape)
    outer, length, inner = int(np.prod(shape[:dim], dtype=np.int64)), shape[dim], int(np.prod(shape[dim + 1:], dtype=np.int64))
    before = x_dev.clone()
    out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    mm = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
    w = np.ascontiguousarray(w, dtype=np.float32)
    st = lib.saber_k_correlate1d_zero(_ptr(x_dev), dtype, _ptr(out), outer, length, inner, w.ctypes.data_as(C.POINTER(C.c_float)), len(w), chunk_len,
                                      _ptr(mm) if minmax else None, None)
    assert st == 0, lib.saber_k_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x_dev.view(torch.uint8), before.view(torch.uint8)), "the kernel wrote its input"
    return out, mm


def _volume_f32(shape, seed):
    """float32 values of mixed sign and scale, with whole columns (every index of each axis) of zeros so that B = 0 somewhere"""
    rng = np.random.default_rng(seed)
    x = (rng.normal(0, 1, shape) * rng.choice([1e-3, 1.0, 3e4], shape)).astype(np.float32)
    x[:, shape[1] // 2, :] = 0
    x[:, :, shape[2] // 3] = 0
    x[shape[0] // 2] *= (rng.random(shape[1:]) > 0.5)
    return x


def _fp64_reference(x, w, dim):
    from scipy.ndimage import correlate1d
    w64 = w.astype(np.float64)
    ref = correlate1d(x.astype(np.float64), w64, axis=dim, mode="constant", cval=0.0)
    bound = (len(w) + 1) * 2.0 ** -24 * correlate1d(np.abs(x.astype(np.float64)), np.abs(w64), axis=dim, mode="constant", cval=0.0)
    return ref, bound


# (shape, dim, sigma, chunk_len): Z < ks with every edge; odd inner * outer (scalar lanes, unaligned rows); halo seams of the automatic
# chunks (at most 32 outputs) on the scalar and on the 16-byte lanes; Z = one chunk + 1; many 8-output chunks; several blocks; dim 1 with
# scalar and 16-byte lanes and outer > 1; dim 2 (the row kernel); ks = 3 and ks = 21 (the kernel for every tap count but 15)
SMOOTH_CASES = [
    ((5, 3, 7), 0, 5, 0),
    ((15, 23, 37), 0, 5, 0),
    ((67, 23, 37), 0, 5, 0),
    ((67, 23, 37), 0, 5, 8),
    ((33, 16, 24), 0, 5, 0),
    ((33, 16, 24), 0, 5, 32),
    ((130, 64, 96), 0, 5, 0),
    ((9, 40, 33), 1, 5, 0),
    ((6, 40, 32), 1, 5, 0),
    ((9, 40, 33), 2, 5, 0),
    ((15, 23, 37), 0, 1, 0),
    ((15, 23, 37), 0, 7, 0),
]


@functools.lru_cache(maxsize=None)
def _smoothed(lib_id, case):
    """one launch per case, shared by the tests below: (input, fp32 taps, device output, device min / max)"""
    shape, dim, sigma, chunk_len = case
    x = _volume_f32(shape, seed=sum(shape) + dim)
    w = _taps(sigma)
    out, mm = _correlate(_LIB[lib_id], _to_dev(x), F32, w, dim, chunk_len)
    return x, w, out, mm


_LIB = {}


def _case(gpu_lib, case):
    _LIB[id(gpu_lib)] = gpu_lib
    return _smoothed(id(gpu_lib), case)


@pytest.mark.parametrize("case", SMOOTH_CASES, ids=lambda c: "x".join(map(str, c[0])) + f"-dim{c[1]}-s{c[2]}-c{c[3]}")
def test_smoothing_against_fp64(gpu_lib, case):
    x, w, out, _ = _case(gpu_lib, case)
    assert len(w) == {5: 15, 1: 3, 7: 21}[case[2]]
    ref, bound = _fp64_reference(x, w, case[1])
    dev = out.cpu().numpy().astype(np.float64)
    err = np.abs(dev - ref)
    frac = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"correlate1d_zero {case}: largest |dev - ref| / B = {frac:.3f}")
    assert (bound == 0).any() and (bound > 0).any()
    assert (err <= bound).all()
    assert (dev[bound == 0] == 0).all()


@pytest.mark.parametrize("case", SMOOTH_CASES, ids=lambda c: "x".join(map(str, c[0])) + f"-dim{c[1]}-s{c[2]}-c{c[3]}")
def test_fused_minmax_equals_aminmax_of_the_output(gpu_lib, case):
    _, _, out, mm = _case(gpu_lib, case)
    lo, hi = torch.aminmax(out)
    assert mm[0].item() == lo.item() and mm[1].item() == hi.item()


def test_chunking_does_not_change_the_bits(gpu_lib):
    """every split of `len` and both lane widths evaluate the same fma chain"""
    x, w, out, _ = _case(gpu_lib, ((67, 23, 37), 0, 5, 0))
    _, _, out8, _ = _case(gpu_lib, ((67, 23, 37), 0, 5, 8))
    assert torch.equal(out.view(torch.int32), out8.view(torch.int32))
    whole, _ = _correlate(gpu_lib, _to_dev(x), F32, w, 0, chunk_len=1 << 20, minmax=False)
    assert torch.equal(out.view(torch.int32), whole.view(torch.int32))


@pytest.mark.parametrize("shape,dim", [((15, 23, 37), 0), ((33, 16, 24), 0), ((6, 40, 32), 1), ((9, 40, 33), 2)], ids=["scalar", "vector", "vector-dim1", "rows"])
@pytest.mark.parametrize("name", ["int16", "uint16", "uint8"])
def test_integer_input_is_widened_exactly(gpu_lib, name, shape, dim):
    """the MRC integer modes give the bits of the float32 run on the widened values"""
    np_dtype, code, lo, hi = {"int16": (np.int16, I16, -32768, 32767), "uint16": (np.uint16, U16, 0, 65535), "uint8": (np.uint8, U8, 0, 255)}[name]
    rng = np.random.default_rng(3)
    x = rng.integers(lo, hi + 1, shape).astype(np_dtype)
    x[:, :, 1] = 0
    x.flat[0], x.flat[-1], x.flat[x.size // 2] = lo, hi, hi
    assert x.min() == lo and x.max() == hi
    w = _taps(5)
    out_i, mm_i = _correlate(gpu_lib, _to_dev(x), code, w, dim)
    out_f, mm_f = _correlate(gpu_lib, _to_dev(x.astype(np.float32)), F32, w, dim)
    assert torch.equal(out_i.view(torch.int32), out_f.view(torch.int32))
    assert torch.equal(mm_i.view(torch.int32), mm_f.view(torch.int32))
    ref, bound = _fp64_reference(x, w, dim)
    assert (np.abs(out_i.cpu().numpy().astype(np.float64) - ref) <= bound).all()


def test_offsets_past_2_to_the_31(gpu_lib):
    """a uint8 volume of 2064 x 1024 x 1024 voxels: element offsets pass 2^31 in the last 16 planes and the fp32 output's byte offsets pass
    2^33; the far end, the near end and the min / max are checked on the device against float64"""
    Z, H, W = 2064, 1024, 1024
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randint(0, 256, (Z, H, W), dtype=torch.uint8, device="cuda", generator=g)
    w = _taps(5)
    out, mm = _correlate(gpu_lib, x, U8, w, 0)
    w64 = torch.from_numpy(w.astype(np.float64)).cuda()
    for z0 in (0, Z - 24):
        xs = torch.zeros((24 + 14, H, W), dtype=torch.float64, device="cuda")          # planes z0 - 7 .. z0 + 30, zero outside the volume
        a, b = max(z0 - 7, 0), min(z0 + 31, Z)
        xs[a - (z0 - 7):b - (z0 - 7)] = x[a:b].double()
        ref = sum(w64[k] * xs[k:k + 24] for k in range(15))
        bound = 16 * 2.0 ** -24 * ref                                                   # x >= 0 and w > 0: the sum of |w| |x| is the reference itself
        err = (out[z0:z0 + 24].double() - ref).abs()
        assert bool((err <= bound).all()), (z0, float((err / bound.clamp_min(1e-300)).max()))
        del xs, ref, bound, err
    lo, hi = torch.aminmax(out)
    assert mm[0].item() == lo.item() and mm[1].item() == hi.item()
    del x, out
    torch.cuda.empty_cache()


def test_correlate_refuses_bad_arguments(gpu_lib):
    x = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros_like(x)
    w = (C.c_float * 65)(*([1.0 / 65] * 65))
    for ks in (1, 2, 14, 65):
        assert gpu_lib.saber_k_correlate1d_zero(_ptr(x), F32, _ptr(out), 1, 4, 16, w, ks, 0, None, None) == -1
        assert b"ks" in gpu_lib.saber_k_last_error()
    assert gpu_lib.saber_k_correlate1d_zero(_ptr(x), F32, _ptr(x), 1, 4, 16, w, 15, 0, None, None) == -1
    assert b"separate" in gpu_lib.saber_k_last_error()
    assert gpu_lib.saber_k_correlate1d_zero(_ptr(x), 4, _ptr(out), 1, 4, 16, w, 15, 0, None, None) == -1
    assert gpu_lib.saber_k_project_mean(_ptr(x), 4, 4, 4, 2, 2, _ptr(out), None) == -1          # an empty range
    assert b"non-empty" in gpu_lib.saber_k_last_error()
    assert gpu_lib.saber_k_project_mean(_ptr(x), 4, 4, 4, 3, 5, _ptr(out), None) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ normalise
@pytest.mark.parametrize("case", [SMOOTH_CASES[6], SMOOTH_CASES[1]], ids=["16-byte-lanes", "odd-count"])
def test_normalize_equals_numpy_bit_for_bit(gpu_lib, case):
    from saber_amd.utils import preprocessing as preprocess
    _, _, out, mm = _case(gpu_lib, case)
    S = out.cpu().numpy()
    expect = preprocess.normalize(S)
    assert expect.dtype == np.float32
    v = out.clone()
    assert gpu_lib.saber_k_normalize_minmax(_ptr(v), v.numel(), _ptr(mm), None) == 0, gpu_lib.saber_k_last_error()
    assert np.array_equal(v.cpu().numpy().view(np.uint32), expect.view(np.uint32))
    # a buffer that starts 4 bytes off a 16-byte boundary (the scalar route), with its own min / max
    flat = out.flatten().clone()
    part = flat[1:]
    mm2 = torch.stack(torch.aminmax(part))
    expect2 = preprocess.normalize(part.cpu().numpy())
    assert gpu_lib.saber_k_normalize_minmax(_ptr(part), part.numel(), _ptr(mm2), None) == 0, gpu_lib.saber_k_last_error()
    assert np.array_equal(part.cpu().numpy().view(np.uint32), expect2.view(np.uint32))
    assert flat[0].item() == out.flatten()[0].item()


def test_normalize_of_a_constant_volume_is_zero(gpu_lib):
    v = torch.full((7, 9, 11), 3.5, dtype=torch.float32, device="cuda")
    mm = torch.tensor([3.5, 3.5], dtype=torch.float32, device="cuda")
    assert gpu_lib.saber_k_normalize_minmax(_ptr(v), v.numel(), _ptr(mm), None) == 0, gpu_lib.saber_k_last_error()
    assert not torch.isnan(v).any() and (v == 0).all()


# ------------------------------------------------------------------------------------------------ projection
@pytest.mark.parametrize("hw", [(16, 24), (21, 27)], ids=["16-byte-lanes", "odd-plane"])
def test_projection_equals_numpy_bit_for_bit(gpu_lib, hw):
    from saber_amd.utils import preprocessing as preprocess
    rng = np.random.default_rng(5)
    vol = (rng.normal(0.4, 0.2, (64,) + hw) * rng.choice([1e-4, 1.0, 50.0], (64,) + hw)).astype(np.float32)
    dev = torch.from_numpy(vol).cuda()
    keep = dev.clone()
    # (zSlice, deltaZ): inside, clipped at z = 0, clipped at z = Z, one plane (deltaZ None), the whole volume (zSlice None), a one-plane range
    for zs, dz in ((32, 10), (3, 10), (60, 10), (17, None), (None, None), (None, 4), (0, 1), (63, 1)):
        expect = np.ascontiguousarray(preprocess.project_tomogram(vol, zs, dz))
        got = preprocess.project_tomogram(dev, zs, dz)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == hw and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().view(np.uint32), expect.view(np.uint32)), (zs, dz)
    assert torch.equal(dev, keep)
    with pytest.raises(RuntimeError, match="non-empty"):
        preprocess.project_tomogram(dev, 70, 3)


# ------------------------------------------------------------------------------------------------ public functions
def test_public_gaussian_smoothing(gpu_lib):
    from saber_amd.filters import gaussian_smoothing
    from saber_amd.filters.gaussian import gaussian_smoothing as same
    assert same is gaussian_smoothing
    x = _volume_f32((9, 40, 33), seed=21)
    w = _taps(5)
    for dim in (-1, 0, 1):
        ref, bound = _fp64_reference(x, w, dim % 3)
        out_np = gaussian_smoothing(x, 5, dim=dim)
        assert isinstance(out_np, np.ndarray) and out_np.dtype == np.float32 and out_np.shape == x.shape
        assert (np.abs(out_np.astype(np.float64) - ref) <= bound).all()
        t = torch.from_numpy(x).cuda()
        out_t = gaussian_smoothing(t, 5, dim=dim)
        assert isinstance(out_t, torch.Tensor) and out_t.device == t.device and out_t.dtype == torch.float32
        assert np.array_equal(out_t.cpu().numpy().view(np.uint32), out_np.view(np.uint32))
        assert torch.equal(t.cpu(), torch.from_numpy(x))
    assert gaussian_smoothing(x, 5).shape == x.shape                        # dim defaults to -1
    ref, bound = _fp64_reference(x, _taps(2), 2)                            # another sigma (ks = 7)
    assert (np.abs(gaussian_smoothing(x, 2).astype(np.float64) - ref) <= bound).all()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        gaussian_smoothing(torch.from_numpy(x), 5)


def test_public_normalize_returns_a_new_tensor(gpu_lib):
    from saber_amd.utils import preprocessing as preprocess
    x = _volume_f32((15, 23, 37), seed=8)
    t = torch.from_numpy(x).cuda()
    out = preprocess.normalize(t)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.data_ptr() != t.data_ptr()
    assert torch.equal(t.cpu(), torch.from_numpy(x))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), preprocess.normalize(x).view(np.uint32))
    again = preprocess.normalize_(t)
    assert again is t and torch.equal(t.view(torch.int32), out.view(torch.int32))
    with pytest.raises(TypeError):
        preprocess.normalize(t, rgb=True)
    with pytest.raises(TypeError):
        preprocess.normalize(t.double())


# ------------------------------------------------------------------------------------------------ end to end
def _tomogram(Z=5, S=384):
    """the toy tomogram of tests/test_gpu_dropin.py"""
    rng = np.random.default_rng(11)
    vol = rng.normal(32768, 3000, (Z, S, S))
    zz, yy, xx = np.mgrid[:Z, :S, :S]
    for _ in range(9):
        cy, cx, r = rng.integers(40, S - 40, 2).tolist() + [int(rng.integers(15, 60))]
        vol[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += rng.choice([-6000, 6000])
    return np.clip(vol, 0, 65535).astype(np.float32)


def _segmenter(cls):
    import os
    os.environ["SABER_AMD_SEEDED_WEIGHTS"] = "1"               # no checkpoint offline: deterministic synthetic weights
    from saber_amd.adapters.base import SAM2AdapterConfig
    from saber_amd.adapters.sam2.amg import cfgAMG
    amg = cfgAMG(npoints=8, crop_n_layers=0, pred_iou_thresh=0.2, stability_score_thresh=0.3, sam2_cfg="small")
    seg = cls(deviceID=0, cfg=SAM2AdapterConfig(cfg="tiny", amg_cfg=amg, min_mask_area=50), min_mask_area=50)
    seg.filter_threshold = -1.0                                # keep every frame: the untrained object-score head says nothing about presence
    return seg


@pytest.fixture(scope="module")
def tomo_segmenter():
    from saber_amd.segmenters.tomo import tomoSegmenter
    return _segmenter(tomoSegmenter)


def test_segment_slab_on_a_device_tensor(gpu_lib, tomo_segmenter):
    """segment_slab keeps the prepared volume on the device; the slab image gives the masks its host copy gives, and the video path builds
    the same frames from the device volume as from its host copy"""
    seg = tomo_segmenter
    vol = _tomogram()
    tv = torch.from_numpy(vol).cuda()
    masks = [m["segmentation"].copy() for m in seg.segment_slab(tv, 2, 2, display=False)]
    assert torch.equal(tv.cpu(), torch.from_numpy(vol))
    assert isinstance(seg.vol, torch.Tensor) and seg.vol.is_cuda and seg.vol.dtype == torch.float32 and tuple(seg.vol.shape) == vol.shape
    vol_h, image0_h = seg.vol.cpu().numpy(), seg.image0.cpu().numpy()
    assert image0_h.shape == vol.shape[1:] and vol_h.min() == 0.0 and 0.99 < vol_h.max() <= 1.0
    # the preparation itself, against the host route's arithmetic on the same data
    from saber_amd.utils import preprocessing as preprocess
    w = _taps(5)
    ref, bound = _fp64_reference(vol, w, 0)
    S, mm = _correlate(gpu_lib, tv, F32, w, 0)
    assert (np.abs(S.cpu().numpy().astype(np.float64) - ref) <= bound).all()
    assert np.array_equal(vol_h.view(np.uint32), preprocess.normalize(S.cpu().numpy()).view(np.uint32))
    assert np.array_equal(image0_h.view(np.uint32), np.ascontiguousarray(preprocess.project_tomogram(vol_h, 2, 2)).view(np.uint32))
    host_masks = seg.segment_image(image0_h, display=False, text_prompt=None, target_class=1)
    assert len(masks) == len(host_masks) > 0
    for a, b in zip(masks, host_masks):
        assert np.array_equal(a, b["segmentation"])
    seg.adapter.set_volume(seg.vol)
    frames_dev = seg.adapter.inference_state.images.clone()
    seg.adapter.set_volume(vol_h)
    frames_host = seg.adapter.inference_state.images
    assert frames_dev.shape == (5, 1024, 1024) and torch.equal(frames_dev.view(torch.int32), frames_host.view(torch.int32))
    assert np.array_equal(seg.vol.cpu().numpy().view(np.uint32), vol_h.view(np.uint32)), "set_volume changed the device volume"
    seg.adapter.reset_state()


def test_segment_vol_on_a_device_tensor(tomo_segmenter):
    seg = tomo_segmenter
    vol = _tomogram()
    tv = torch.from_numpy(vol).cuda()
    out = seg.segment_vol(tv, thickness=2, zSlice=2)
    assert out is not None and isinstance(out, np.ndarray) and out.shape == vol.shape and out.dtype == np.uint16
    assert out[2].any(), "the seeded frame lost its masks"
    assert set(seg.adapter.frame_metrics) == set(range(5))
    assert torch.equal(tv.cpu(), torch.from_numpy(vol))
    u16 = _to_dev(vol.astype(np.uint16))                       # an MRC integer mode goes the same way (the toy tomogram holds whole numbers only after this cast)
    out16 = seg.segment_vol(u16, thickness=2, zSlice=2)
    assert out16 is not None and out16.shape == vol.shape and out16.dtype == np.uint16
    with pytest.raises(TypeError):
        seg.segment_slab(tv.double(), 2, 2, display=False)


def test_segment_tomogram_core_with_device_prep(tomo_segmenter):
    import types
    from saber_amd.entry_points.inference_core import segment_tomogram_core
    seg = tomo_segmenter
    vol = _tomogram()
    written = {}

    def read(run, voxel_size, algorithm=None):
        return vol

    def write(run, mask, user, name=None, session_id=None, voxel_size=None):
        written[run.name] = (mask, user, name, session_id, voxel_size)

    run = types.SimpleNamespace(name="run1")
    assert segment_tomogram_core(run, 10.0, "wbp", "organelles", "1", 2, 1, 0, False, seg, gpu_id=0, read_tomogram=read, write_segmentation=write,
                                 device_prep=True) is None
    mask, user, name, sid, vs = written["run1"]
    assert mask.shape == vol.shape and mask.dtype == np.uint8 and (user, name, sid, vs) == ("saber", "organelles", "1", 10.0)
    assert isinstance(seg.vol, torch.Tensor) and seg.vol.is_cuda, "device_prep did not take the device route"
    assert seg.inference_state is None


def test_multi_depth_segmenter_on_a_device_tensor():
    from saber_amd.segmenters.tomo import multiDepthTomoSegmenter
    seg = _segmenter(multiDepthTomoSegmenter)
    vol = _tomogram()
    tv = torch.from_numpy(vol).cuda()
    out = seg.segment(tv, thickness=2, num_slabs=2, delta_z=1)
    assert out.shape == vol.shape and out.dtype == np.uint32
    assert torch.equal(tv.cpu(), torch.from_numpy(vol)), "the input changed between slabs"
