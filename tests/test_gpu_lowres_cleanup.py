"""GPU: the clean-up of the low-resolution mask logits on the device (csrc/lowres_cleanup.hip: saber_k_clean_lowres, Engine.clean_lowres,
Engine.set_lowres_cleanup / the amg_generate keywords) - upstream's SAM2ImagePredictor(max_hole_area=.., max_sprinkle_area=..).
  (a) the kernel against the scipy restatement (tests/lowres_cleanup_ref.py), BIT FOR BIT (uint32 views), on every shape and content of
      kernel_cases(); index map and pass flags; two calls give equal bytes; error paths leave the buffer alone;
  (b) the generator on the fitted decoder: 0 / 0 is the handle that never heard of the option; the device route equals the host route
      with the option on; the masks are K8 over the planes of decode_points cleaned by the RESTATEMENT; the m2m pass still reads the
      uncleaned first-pass planes."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import lowres_cleanup_ref as R

pytestmark = pytest.mark.gpu


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def clean(gpu_lib, x, thr, h, s, idx=None, flags=None, n=None):
    """x: (P,H,W) float32 numpy -> what the device made of it"""
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    di = torch.from_numpy(np.asarray(idx, np.int32)).cuda() if idx is not None else None
    df = torch.from_numpy(np.asarray(flags, np.uint8)).cuda() if flags is not None else None
    st = gpu_lib.saber_k_clean_lowres(ptr(d), ptr(di), ptr(df), x.shape[0] if n is None else n, x.shape[1], x.shape[2], float(thr), int(h), int(s), None)
    assert st == 0, gpu_lib.saber_k_last_error()
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    """every case with its reference, computed once"""
    return [(name, x, thr, h, s, R.clean_lowres_ref(x, thr, h, s)) for (name, x, thr, h, s) in R.kernel_cases()]


# ------------------------------------------------------------------------------------------------ (a) the kernel
def test_kernel_equals_restatement_bit_for_bit(gpu_lib, cases):
    bad = []
    changed = 0
    for name, x, thr, h, s, ref in cases:
        got = clean(gpu_lib, x, thr, h, s)
        changed += int((R.bits(ref) != R.bits(x)).sum())
        if not np.array_equal(R.bits(got), R.bits(ref)):
            bad.append((name, int((R.bits(got) != R.bits(ref)).sum())))
    print(f"{len(cases)} cases, {changed} pixels changed by the restatement in all")
    assert changed > 0
    assert not bad, bad


def test_two_calls_give_equal_bytes(gpu_lib):
    x = R.noise(11, 6, 256, 256)
    a = clean(gpu_lib, x, 0.0, 25, 25)
    b = clean(gpu_lib, x, 0.0, 25, 25)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(R.bits(a), R.bits(R.clean_lowres_ref(x, 0.0, 25, 25)))
    # cleaning the result again with the same areas changes nothing more than the restatement says (it is no fixed point in general)
    assert np.array_equal(R.bits(clean(gpu_lib, a, 0.0, 25, 25)), R.bits(R.clean_lowres_ref(a, 0.0, 25, 25)))


def test_many_planes_more_than_compute_units(gpu_lib):
    x = R.noise(5, 300, 64, 100)                                   # more workgroups than the device has CUs
    assert np.array_equal(R.bits(clean(gpu_lib, x, 0.0, 12, 30)), R.bits(R.clean_lowres_ref(x, 0.0, 12, 30)))


@pytest.mark.parametrize("shape", [(17, 33), (256, 256)])
def test_index_map_and_pass_flags(gpu_lib, shape):
    """plane k of the call is idx[k]; pass[k] == 0 skips it: unflagged and unindexed planes keep a sentinel bit pattern"""
    H, W = shape
    P = 9
    x = R.noise(3, P, H, W)
    sentinel = np.float32(np.frombuffer(np.uint32(0x7fc12345).tobytes(), np.float32)[0])      # a NaN with a payload: no kernel writes it, and a kernel that ran keeps it
    idx = np.array([7, 2, 5, 0, 3], np.int32)                      # planes 1, 4, 6, 8 are not indexed
    flags = np.array([1, 0, 1, 1, 0], np.uint8)                    # planes 2 and 3 are indexed but not flagged
    live = [7, 5, 0]
    for p in range(P):
        if p not in live:
            x[p, ::2, ::3] = sentinel                              # in planes nothing may touch: a plane that was cleaned by mistake shows around them
    ref = x.copy()
    ref[live] = R.clean_lowres_ref(x[live], 0.0, 25, 25)
    got = clean(gpu_lib, x, 0.0, 25, 25, idx=idx, flags=flags, n=len(idx))
    assert np.array_equal(R.bits(got), R.bits(ref))
    assert (R.bits(ref[live]) != R.bits(x[live])).any()
    # idx alone: every indexed plane; pass alone: plane k itself
    ref = x.copy()
    ref[idx] = R.clean_lowres_ref(x[idx], 0.0, 25, 25)
    assert np.array_equal(R.bits(clean(gpu_lib, x, 0.0, 25, 25, idx=idx, n=len(idx))), R.bits(ref))
    ref = x.copy()
    on = [k for k in range(len(flags)) if flags[k]]
    ref[on] = R.clean_lowres_ref(x[on], 0.0, 25, 25)
    assert np.array_equal(R.bits(clean(gpu_lib, x, 0.0, 25, 25, flags=flags, n=len(flags))), R.bits(ref))


def test_error_paths_leave_the_buffer_untouched(gpu_lib):
    x = R.noise(2, 2, 17, 33)
    d = torch.from_numpy(x).cuda()
    for planes, n, H, W, h, s in ((None, 2, 17, 33, 5, 5), (ptr(d), -1, 17, 33, 5, 5), (ptr(d), 2, 0, 33, 5, 5), (ptr(d), 2, 17, 0, 5, 5),
                                  (ptr(d), 2, 257, 256, 5, 5), (ptr(d), 2, 17, 33, -1, 5), (ptr(d), 2, 17, 33, 5, 65536), (ptr(d), 2, 17, 33, 65536, 0)):
        assert gpu_lib.saber_k_clean_lowres(planes, None, None, n, H, W, 0.0, h, s, None) == -1
        assert gpu_lib.saber_k_last_error().decode().startswith("clean_lowres:")
    # nothing to do: status 0, no launch
    assert gpu_lib.saber_k_clean_lowres(ptr(d), None, None, 0, 17, 33, 0.0, 5, 5, None) == 0
    assert gpu_lib.saber_k_clean_lowres(ptr(d), None, None, 2, 17, 33, 0.0, 0, 0, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(d.cpu().numpy()), R.bits(x))


def test_engine_wrapper(gpu_lib):
    from saber_amd.engine import Engine
    eng = Engine.bare(0)
    try:
        x = R.noise(4, 3, 256, 256)
        d = torch.from_numpy(x).cuda()
        out = eng.clean_lowres(d, 25, 9, mask_threshold=0.5)
        assert out is d                                            # in place
        torch.cuda.synchronize()
        assert np.array_equal(R.bits(d.cpu().numpy()), R.bits(R.clean_lowres_ref(x, 0.5, 25, 9)))
        with pytest.raises(ValueError, match="max_hole_area"):
            eng.clean_lowres(d, -1, 0)
        with pytest.raises(ValueError, match="float32"):
            eng.clean_lowres(d.double(), 1, 1)
        with pytest.raises(ValueError, match="clean_lowres:"):
            eng.clean_lowres(torch.zeros((1, 300, 300), device="cuda"), 1, 1)
        assert eng.clean_lowres(d[:0], 1, 1).shape[0] == 0
        with pytest.raises(ValueError, match="set_lowres_cleanup"):
            eng._check(eng.lib.saber_engine_set_lowres_cleanup(eng.h, 70000, 0))
        eng.set_lowres_cleanup(3, 4)
        eng.set_lowres_cleanup(0, 0)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ (b) the generator
A = 25          # upstream's generator passes min_mask_region_area to both areas; SABER's value is 25
ALL_PASS = dict(npoints=4, crop_n_layers=0, pred_iou_thresh=0.0, stability_score_thresh=0.0, box_nms_thresh=1.0, multimask_output=True)


def fitted_handle():
    """a handle on the seeded encoder with the fitted mask decoder (tests/test_gpu_fitted_decoder.py), and its prepared test slice"""
    from oracle import saber_ref
    from saber_amd.engine import Engine
    from saber_amd.model_config import get_config
    from saber_amd.weights import fitted_decoder_weights
    eng = Engine("large", device=0, weights=fitted_decoder_weights(get_config("large"), 0), max_images=5, max_prompts=64)
    return eng, eng.prepare(torch.from_numpy(saber_ref.synthetic_slice(seed=0)).cuda())


@pytest.fixture(scope="module")
def fitted():
    eng, img = fitted_handle()
    yield eng, img
    eng.close()


def generate(eng, img, amg, **kw):
    from saber_amd.engine import make_amg_params
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        bits, meta = eng.amg_generate(img, make_amg_params(amg), max_masks=1024, **kw)
        st.synchronize()
    return bits.cpu().numpy().view(np.uint32), b"".join(bytes(m) for m in meta), meta


def rows_multiset(bits):
    return sorted(r.tobytes() for r in bits)


def test_off_is_the_handle_that_never_called_the_setter(fitted):
    eng, img = fitted
    amg = dict(npoints=8, crop_n_layers=1)
    fresh, fresh_img = fitted_handle()
    try:
        base_bits, base_rec, meta = generate(fresh, fresh_img, amg)
    finally:
        fresh.close()
    assert len(meta) >= 3
    eng.set_lowres_cleanup(A, A)
    on_bits, on_rec, _ = generate(eng, img, amg)
    eng.set_lowres_cleanup(0, 0)
    off_bits, off_rec, _ = generate(eng, img, amg)
    assert off_rec == base_rec and np.array_equal(off_bits, base_bits)
    kw_bits, kw_rec, _ = generate(eng, img, amg, max_hole_area=0, max_sprinkle_area=0)
    assert kw_rec == base_rec and np.array_equal(kw_bits, base_bits)
    # the keywords are the setter for one call
    k_bits, k_rec, _ = generate(eng, img, amg, max_hole_area=A, max_sprinkle_area=A)
    assert k_rec == on_rec and np.array_equal(k_bits, on_bits)
    off_bits, off_rec, _ = generate(eng, img, amg)
    assert off_rec == base_rec and np.array_equal(off_bits, base_bits)


@pytest.mark.parametrize("use_m2m", [False, True])
def test_device_route_equals_host_route_with_the_option_on(fitted, use_m2m):
    eng, img = fitted
    amg = dict(npoints=8, crop_n_layers=1, use_m2m=use_m2m, pred_iou_thresh=0.5, stability_score_thresh=0.8)
    try:
        eng.set_lowres_cleanup(A, A)
        dev_bits, dev_rec, meta = generate(eng, img, amg)
        eng.set_device_amg(False)
        host_bits, host_rec, _ = generate(eng, img, amg)
    finally:
        eng.set_device_amg(True)
        eng.set_lowres_cleanup(0, 0)
    print(f"use_m2m {use_m2m}: {len(meta)} masks with the option on")
    assert len(meta) >= 3
    assert dev_rec == host_rec and np.array_equal(dev_bits, host_bits)


def grid_points(n):
    """the generator's point grid on the whole 1024 x 1024 image, in model pixels (csrc/amg.hip: float64 grid, float32 from the crop's pixels on)"""
    off = 1.0 / (2.0 * n)
    g = [off + (1.0 - 2.0 * off) * i / (n - 1) for i in range(n)]
    px = np.array([[np.float32(g[ix] * 1024.0), np.float32(g[iy] * 1024.0)] for iy in range(n) for ix in range(n)], np.float32)
    return (px / np.float32(1024.0)) * np.float32(1024.0)


def mask_post(gpu_lib, planes):
    """K8 on (n,256,256) planes for the whole 1024 x 1024 image, at the generator's threshold and stability offset"""
    n = planes.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(planes)).cuda()
    bits = torch.zeros((n, 1024, 32), dtype=torch.int32, device="cuda")
    stats = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    assert gpu_lib.saber_k_mask_post(ptr(d), n, 0, 0, 1024, 1024, 1024, 1024, 0.0, 0.7, ptr(bits), ptr(stats), None) == 0, gpu_lib.saber_k_last_error()
    torch.cuda.synchronize()
    return bits.cpu().numpy().view(np.uint32)


def test_masks_are_k8_over_planes_cleaned_by_the_restatement(gpu_lib, fitted):
    """Every candidate of a 4 x 4 grid comes out (no m2m, all-pass thresholds, NMS off).  Precondition, option off: the generator's mask
    rows are, as a multiset, K8 over the planes decode_points returns for the grid's points.  Check, option on: they are K8 over those
    planes cleaned by the restatement."""
    eng, img = fitted
    amg = dict(ALL_PASS, use_m2m=False)
    off_bits, _, meta = generate(eng, img, amg)
    assert len(meta) == 48
    eng.encode(img)
    low, _, _ = eng.decode_points(torch.from_numpy(grid_points(4)).cuda(), slot=0, multimask=True)
    torch.cuda.synchronize()
    planes = low.cpu().numpy().reshape(48, 256, 256)
    assert rows_multiset(off_bits) == rows_multiset(mask_post(gpu_lib, planes)), "precondition: the generator's decode and decode_points differ"
    cleaned = R.clean_lowres_ref(planes, 0.0, A, A)
    n_changed = int((R.bits(cleaned) != R.bits(planes)).sum())
    on_bits, _, meta_on = generate(eng, img, amg, max_hole_area=A, max_sprinkle_area=A)
    want = mask_post(gpu_lib, cleaned)
    print(f"{n_changed} low-res pixels of 48 planes changed by the restatement at {A}; {int((want != mask_post(gpu_lib, planes)).any(axis=(1, 2)).sum())} masks differ")
    assert len(meta_on) == 48
    assert rows_multiset(on_bits) == rows_multiset(want)
    # only-holes and only-sprinkles are their own options
    for h, s in ((A, 0), (0, A)):
        bits_hs, _, _ = generate(eng, img, amg, max_hole_area=h, max_sprinkle_area=s)
        assert rows_multiset(bits_hs) == rows_multiset(mask_post(gpu_lib, R.clean_lowres_ref(planes, 0.0, h, s)))


def test_m2m_pass_reads_the_uncleaned_first_pass_planes(fitted):
    """with use_m2m the refinement pass's planes are cleaned; the first-pass planes feed its mask prompt untouched, so its IoU predictions
    are those of the option-off run"""
    eng, img = fitted
    amg = dict(ALL_PASS, use_m2m=True)
    off_bits, _, off_meta = generate(eng, img, amg)
    on_bits, _, on_meta = generate(eng, img, amg, max_hole_area=A, max_sprinkle_area=A)
    assert len(off_meta) == 48 and len(on_meta) == 48
    key = lambda meta: sorted(np.float32(m.predicted_iou).tobytes() for m in meta)
    assert key(on_meta) == key(off_meta)
    print(f"m2m: {int(sum(a != b for a, b in zip(rows_multiset(on_bits), rows_multiset(off_bits))))} of 48 sorted mask rows differ with the option on")
