"""GPU: the smoothing over z-chunks (csrc/smooth3d.hip: saber_smooth_labels_chunk / saber_smooth_radius / saber_label_max / saber_label_counts;
saber_amd/segmenters/smooth.py) against Engine.smooth_labels on the whole volume.  The chunks' bytes are compared with the whole volume's
bit for bit (torch.equal) for the splits 1, 2, 3 and Z; the whole-volume result itself is held against the reference's fixtures
(tests/golden/saber_smooth.npz) or the oracle under the BAND rule of tests/test_gpu_smooth3d.py: identical outside the voxels where
some label's oracle field lies within 1e-5 of the threshold, and those voxels at most max(8, 0.1 % of the foreground)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import sharded_smooth_ref as ref
from saber_amd.segmenters import smooth

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "saber_smooth.npz"), allow_pickle=False)
BAND = 1e-5


@pytest.fixture(scope="module")
def ctx():
    from saber_amd.engine import Engine
    e = Engine.bare(0)
    yield e
    e.close()


def to_dev(vol):
    v = np.ascontiguousarray(vol)
    return torch.from_numpy(v.view({1: np.uint8, 2: np.int16, 4: np.int32}[v.dtype.itemsize])).cuda()


def check_chunks(ctx, vol, scale, splits=None):
    """smooth_labels_chunks of `vol` for every split against smooth_labels on the whole volume, bit for bit; returns the latter (numpy)"""
    dev = to_dev(vol)
    Z = vol.shape[0]
    whole, _ = ctx.smooth_labels(dev, scale)
    for parts in sorted(set(splits or (1, 2, 3, Z))):
        chunks = [dev[a:b] for a, b in ref.cuts_of(Z, parts)]
        out = smooth.smooth_labels_chunks(ctx, chunks, scale)
        assert all(o.dtype == torch.uint8 and o.is_cuda and o.shape == c.shape for o, c in zip(out, chunks))
        assert torch.equal(torch.cat(out, 0), whole), (vol.shape, scale, parts)
    return whole.cpu().numpy()


def check_band(got, vol, scale, golden=None):
    """the BAND rule (tests/test_gpu_smooth3d.py: check), the cap on the band included"""
    from oracle import saber_ref
    want, near = saber_ref.fast_3d_gaussian_smoothing(vol, scale, band=BAND)
    if golden is not None:
        assert not ((golden != want) & ~near).any()
        want = golden
    assert got.dtype == np.uint8 and got.shape == vol.shape
    bad = (got != want) & ~near
    assert not bad.any(), f"{int(bad.sum())} voxels differ outside the threshold band"
    assert near.sum() <= max(8, 1e-3 * (vol != 0).sum())
    return want, near


@pytest.mark.parametrize("inp,scale,name", [("a_in", 0.075, "a_out_s075"), ("b_in", 0.05, "b_out_s05"), ("c_in", 0.075, "c_out_s075")])
def test_reference_fixtures(ctx, inp, scale, name):
    check_band(check_chunks(ctx, G[inp], scale), G[inp], scale, golden=G[name])


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_blobs(ctx, name):
    """a: (12,40,70) at 0.15, b: (9,33,65) at 0.3 - label values above 255 and above 65535, and from 3 chunks on the halo (radius 5 / 9) is
    deeper than every chunk; c: (20,150,333) at 0.075"""
    vol, scale = ref.blob_case(name)
    check_band(check_chunks(ctx, vol, scale), vol, scale)


def test_sandwich(ctx):
    """label 7 on both sides of plane 4 and not on it: the one-plane chunk of plane 4 must not skip it.  The oracle's band is empty here, so
    the BAND rule asks for the oracle's bytes exactly."""
    vol, scale = ref.sandwich()
    got = check_chunks(ctx, vol, scale)
    want, near = check_band(got, vol, scale)
    assert not near.any() and np.array_equal(got, want) and int((got[4] == 7).sum()) == 304
    own = to_dev(vol[4:5])                                          # the chunk of plane 4 alone, called directly
    out, n = ctx.smooth_labels_chunk(own, to_dev(vol[:4]), to_dev(vol[5:]), [7], [int((vol == 7).sum())], scale, True, True)
    assert n == 1 and np.array_equal(out.cpu().numpy(), want[4:5])
    out, n = ctx.smooth_labels_chunk(own, to_dev(vol[:4]), None, [7], [int((vol == 7).sum())], scale, True, True)
    assert n == 0 and not out.any()                                 # every voxel on one side of the own plane: skipped, and rightly empty


def test_dtypes(ctx):
    a = G["a_in"]
    base = check_chunks(ctx, a, 0.05)                               # int32
    assert np.array_equal(check_chunks(ctx, a.astype(np.uint8), 0.05), base)
    assert np.array_equal(check_chunks(ctx, a.astype(np.uint16), 0.05), base)          # as int16
    hi = a.astype(np.uint16)
    hi[hi == 4] = 40000                                             # beyond int16: the element bytes are read as unsigned
    check_band(check_chunks(ctx, hi, 0.05), hi, 0.05)


def test_empty_chunk_and_zero_volume(ctx):
    vol, scale = ref.blob_case("a")
    dev = to_dev(vol)
    whole, _ = ctx.smooth_labels(dev, scale)
    chunks = [dev[0:5], dev[5:5], dev[5:6], dev[6:12], dev[12:12]]
    out = smooth.smooth_labels_chunks(ctx, chunks, scale)
    assert [tuple(o.shape) for o in out] == [tuple(c.shape) for c in chunks] and torch.equal(torch.cat(out, 0), whole)
    zero = torch.zeros((5, 9, 70), dtype=torch.int32, device="cuda")
    out = smooth.smooth_labels_chunks(ctx, [zero[:2], zero[2:]], scale)
    assert all(o.dtype == torch.uint8 and not o.any() for o in out) and [o.shape[0] for o in out] == [2, 3]
    o, n = ctx.smooth_labels_chunk(zero[:2].contiguous(), None, zero[2:].contiguous(), [], [], scale, True, True)
    assert n == 0 and not o.any()


def test_one_label_whose_radius_exceeds_the_volume(ctx):
    """one label filling (8,64,64) at scale 0.3: radius 36, every halo is the rest of the volume"""
    vol = np.ones((8, 64, 64), np.uint32)
    assert ctx.smooth_radius(vol.size, 0.3) == ref.radius_of(vol.size, 0.3) == 36
    check_band(check_chunks(ctx, vol, 0.3), vol, 0.3)
    slab = np.zeros((8, 64, 64), np.uint32)
    slab[:, 8:56, 8:56] = 3                                         # the same with a border and a smaller scale: something is set
    got = check_chunks(ctx, slab, 0.1)
    assert ctx.smooth_radius(int((slab == 3).sum()), 0.1) > 8 and (got == 3).any()
    check_band(got, slab, 0.1)


def test_radius_is_the_librarys(ctx):
    for scale in (0.05, 0.075, 0.3):
        for count in (1, 2, 7, 100, 4189, 65536, 10 ** 6, 3 * 10 ** 7):
            assert ctx.smooth_radius(count, scale) == ref.radius_of(count, scale), (count, scale)
    assert ctx.smooth_radius(0, 0.05) == 0
    with pytest.raises(ValueError):
        ctx.smooth_radius(-1, 0.05)
    with pytest.raises(ValueError):
        ctx.smooth_radius(5, 0.0)


def test_counts(ctx):
    vol, _ = ref.blob_case("a")
    dev = to_dev(vol)
    m = ctx.label_max(dev)
    assert m == int(vol.max()) == 70000
    counts = ctx.label_counts(dev, m + 1)
    want = np.bincount(vol.ravel(), minlength=m + 1)
    want[0] = 0                                                     # the background is not counted
    assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), want)
    with pytest.raises(ValueError, match="label_counts: label value 70000"):
        ctx.label_counts(dev, 70000)


def test_errors(ctx):
    lib, h = ctx.lib, ctx.h
    own = torch.zeros((2, 8, 70), dtype=torch.int32, device="cuda")
    own[0, 2, 3:9] = 1
    own[1, 4, 60:] = 2
    with pytest.raises(ValueError, match="smooth_labels_chunk: label value 2 is not in the table"):
        ctx.smooth_labels_chunk(own, None, None, [1], [6], 0.05, True, True)
    ok, n = ctx.smooth_labels_chunk(own, None, None, [1, 2, 9], [6, 10, 4], 0.05, True, True)
    assert n == 2 and torch.equal(ok, ctx.smooth_labels(own, 0.05)[0])
    r = ctx.smooth_radius(50000, 0.05)
    assert r > 1
    halo = torch.zeros((1, 8, 70), dtype=torch.int32, device="cuda")
    for lo, hi, lo_end, hi_end in ((halo, None, False, True), (None, halo, True, False), (None, None, False, True)):
        with pytest.raises(ValueError, match="smooth_labels_chunk: a halo of . planes is shorter than the largest radius"):
            ctx.smooth_labels_chunk(own, lo, hi, [1, 2], [50000, 10], 0.05, lo_end, hi_end)
    ctx.smooth_labels_chunk(own, halo, None, [1, 2], [50000, 10], 0.05, True, True)    # the same halo where the volume ends: fine
    with pytest.raises(ValueError, match="smooth_labels_chunk: the table must list ascending"):
        ctx.smooth_labels_chunk(own, None, None, [2, 1], [6, 10], 0.05, True, True)
    with pytest.raises(ValueError, match="smooth_labels_chunk: label values above 2\\^22"):
        ctx.smooth_labels_chunk(own, None, None, [1, 2, (1 << 22) + 1], [6, 10, 1], 0.05, True, True)
    with pytest.raises(ValueError, match="smooth_labels_chunk: Gaussian radius"):
        ctx.smooth_labels_chunk(own, None, None, [1, 2], [6, 10 ** 9], 0.3, True, True)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty((2, 8, 70), dtype=torch.uint8, device="cuda")
    assert lib.saber_smooth_labels_chunk(h, None, 0, p(own), 0, None, 0, 1, 1, 4, 8, 70, None, None, 0, 0.05, p(out), None, st) == -1
    assert b"smooth_labels_chunk:" in lib.saber_last_error(h)
    assert lib.saber_smooth_labels_chunk(h, None, 0, p(own), 1 << 11, None, 0, 1, 1, 4, 1 << 10, 1 << 10, None, None, 0, 0.05, p(out), None, st) == -1
    assert b"smooth_labels_chunk:" in lib.saber_last_error(h) and b"2^31" in lib.saber_last_error(h)
    # the wrappers' own checks
    with pytest.raises(ValueError, match="smooth_labels_chunk: lo has planes of"):
        ctx.smooth_labels_chunk(own, own[:, :4].contiguous(), None, [1, 2], [6, 10], 0.05, True, True)
    with pytest.raises(ValueError, match="smooth_labels_chunk: hi is"):
        ctx.smooth_labels_chunk(own, None, own.to(torch.int16), [1, 2], [6, 10], 0.05, True, True)
    with pytest.raises(ValueError, match="smooth_labels_chunk: own must be"):
        ctx.smooth_labels_chunk(own.cpu(), None, None, [1, 2], [6, 10], 0.05, True, True)
    with pytest.raises(ValueError, match="smooth_labels_chunk: 2 ids and 1 counts"):
        ctx.smooth_labels_chunk(own, None, None, [1, 2], [6], 0.05, True, True)
    with pytest.raises(ValueError, match="smooth_labels_chunks: every chunk must be \\(Zc,H,W\\) with the same H and W"):
        smooth.smooth_labels_chunks(ctx, [own, own[:, :4].contiguous()], 0.05)
    with pytest.raises(ValueError, match="smooth_labels_chunks: no chunks"):
        smooth.smooth_labels_chunks(ctx, [], 0.05)


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_driver_single_process(ctx):
    from saber_amd.segmenters.slice_driver import segment_volume_sharded
    from sharded_stitch_worker import planes_of
    vol = planes_of(5)
    dev = torch.from_numpy(vol.view(np.int16)).cuda()
    fn = lambda z: dev[z]
    want = segment_volume_sharded(vol, fn, min_mask_area=1, engine=ctx, smooth_scale=0.05)          # the gathered route
    assert want.dtype == np.uint8 and want.any()
    t = {}
    out = segment_volume_sharded(vol, fn, min_mask_area=1, engine=ctx, sharded_stitch=True, sharded_smooth=0.05, timings=t)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and np.array_equal(out, want)
    assert {"stitched", "counted", "halos", "smoothed", "gathered"} <= set(t)
    chunk, span = segment_volume_sharded(vol, fn, min_mask_area=1, engine=ctx, sharded_stitch=True, sharded_smooth=0.05, gather="none")
    assert span == (0, 5) and chunk.is_cuda and chunk.dtype == torch.uint8 and np.array_equal(chunk.cpu().numpy(), want)
    kept = segment_volume_sharded(vol, fn, min_mask_area=1, engine=ctx, sharded_stitch=True, sharded_smooth=0.05, keep_on_device=True)
    assert kept.is_cuda and np.array_equal(kept.cpu().numpy(), want)
    with pytest.raises(ValueError, match="smooth_scale needs the whole volume"):                    # the old combination still raises
        segment_volume_sharded(vol, fn, engine=ctx, sharded_stitch=True, smooth_scale=0.05)
    with pytest.raises(ValueError, match="sharded_smooth needs sharded_stitch"):
        segment_volume_sharded(vol, fn, engine=ctx, sharded_smooth=0.05)
    with pytest.raises(ValueError, match="sharded_smooth needs sharded_stitch"):
        segment_volume_sharded(vol, fn, sharded_stitch=True, sharded_smooth=0.05)
    with pytest.raises(ValueError, match="sharded_smooth needs the planes on the engine's device"):
        segment_volume_sharded(vol, lambda z: dev[z].cpu(), engine=ctx, sharded_stitch=True, sharded_smooth=0.05)


def test_two_gloo_ranks_on_one_device(tmp_path):
    """two gloo ranks on this one GPU with weight-less handles: device planes, collectives and halos staged through the host; Z = 7 (chunks
    of 4 + 3 planes) and Z = 1 (the second rank owns nothing).  The whole-volume result is the workers' own (host stitch, then
    Engine.smooth_labels on the whole volume): this process starts no GPU work, two processes use the device."""
    from saber_amd.segmenters.slice_driver import shard_bounds
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sharded_smooth_worker.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    procs = []
    for r in range(2):                                              # the ranks meet at the rendezvous: both have to be running
        e = dict(env, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(30100 + os.getpid() % 200))
        procs.append(subprocess.Popen([sys.executable, worker, str(tmp_path / f"r{r}.npz")], env=e))
    status = []
    try:
        for p_ in procs:
            status.append(p_.wait(timeout=180))
    finally:
        for p_ in procs:
            if p_.poll() is None:
                p_.kill()
                p_.wait()
    assert status == [0, 0], status
    got = [np.load(str(tmp_path / f"r{r}.npz")) for r in range(2)]
    for Z in (7, 1):
        want = got[0][f"whole{Z}"]
        assert want.dtype == np.uint8 and want.shape == (Z, 40, 48) and want.any() and np.array_equal(got[1][f"whole{Z}"], want)
        for r in range(2):
            a, b = shard_bounds(Z, 2, r)
            assert np.array_equal(got[r][f"all{Z}"], want) and np.array_equal(got[r][f"kept{Z}"], want), (Z, r)
            assert got[r][f"none{Z}"].dtype == np.uint8 and np.array_equal(got[r][f"none{Z}"], want[a:b]), (Z, r)
        assert np.array_equal(got[0][f"rank0{Z}"], want)


# ---------------------------------------------------------------------------------------------------------------- one size check
def test_volume_scale_eight_chunks(ctx, tmp_path):
    """the 64 x 1024 x 1024 volume of 150 balls of tests/test_gpu_smooth3d.py::test_volume_scale_locality in 8 chunks of 8 planes: the
    chunks' bytes are the whole volume's.  Prints one timing line (the 8 chunks run one after the other on the one device) and writes
    it to sharded_smooth_timing.txt in the directory SABER_AMD_TIMING_DIR names (default: the test's temporary directory)."""
    rng = np.random.default_rng(9)
    Z, H, W = 64, 1024, 1024
    vol = torch.zeros((Z, H, W), dtype=torch.int32, device="cuda")
    for k in range(150):                                            # the same draws; every ball is painted inside its own box
        cz, cy, cx, r = int(rng.integers(0, Z)), int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(8, 60))
        lo = [max(c - r, 0) for c in (cz, cy, cx)]
        hi = [min(c + r + 1, n) for c, n in zip((cz, cy, cx), (Z, H, W))]
        g = [torch.arange(a, b, device="cuda") - c for a, b, c in zip(lo, hi, (cz, cy, cx))]
        inside = (g[0].view(-1, 1, 1) ** 2 + g[1].view(1, -1, 1) ** 2 + g[2].view(1, 1, -1) ** 2) < r * r
        vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].masked_fill_(inside, k + 1)
    chunks = [vol[a:b] for a, b in ref.cuts_of(Z, 8)]
    whole, n = ctx.smooth_labels(vol, 0.05)                         # also the warm-up of the shared kernels
    smooth.smooth_labels_chunks(ctx, chunks, 0.05)
    torch.cuda.synchronize()
    t0 = time.time()
    whole, n = ctx.smooth_labels(vol, 0.05)
    torch.cuda.synchronize()
    t1 = time.time()
    out = smooth.smooth_labels_chunks(ctx, chunks, 0.05)
    torch.cuda.synchronize()
    t2 = time.time()
    assert torch.equal(torch.cat(out, 0), whole) and n > 100 and whole.any()
    line = (f"smooth_labels 64x1024x1024 int32, {n} labels: whole {(t1 - t0) * 1e3:.1f} ms; 8 chunks of 8 planes one after the other "
            f"(count, halo slices, chunk call) {(t2 - t1) * 1e3:.1f} ms in all")
    print("\n" + line)
    out_dir = os.environ.get("SABER_AMD_TIMING_DIR") or str(tmp_path)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "sharded_smooth_timing.txt"), "w") as f:
        f.write(line + "\n")
