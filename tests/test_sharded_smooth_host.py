"""CPU: the host side of the sharded smoothing (saber_amd/segmenters/smooth.py) - the halo plan, the point-to-point halo exchange under
gloo - and the numpy restatement of the scheme (tests/sharded_smooth_ref.py) against the oracle on the whole volume, byte for byte."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sharded_smooth_ref as ref
from oracle import saber_ref
from saber_amd.segmenters import smooth
from saber_amd.segmenters.slice_driver import shard_bounds


# ---------------------------------------------------------------------------------------------------------------- halo_plan
@pytest.mark.parametrize("Z,world,h", [(7, 2, 2), (8, 3, 5), (2, 3, 4), (7, 2, 0), (8, 3, 0), (2, 3, 0)])
def test_halo_plan(Z, world, h):
    bounds = [shard_bounds(Z, world, r) for r in range(world)]
    owner = {z: q for q, (a, b) in enumerate(bounds) for z in range(a, b)}
    plans = [smooth.halo_plan(bounds, r, h) for r in range(world)]
    for r, ((z0, z1), p) in enumerate(zip(bounds, plans)):
        want = {"lo": list(range(max(z0 - h, 0), z0)), "hi": list(range(z1, min(z1 + h, Z)))} if z1 > z0 else {"lo": [], "hi": []}
        for side in ("lo", "hi"):
            got = [z for q, a, b in p[side] for z in range(a, b)]
            assert got == want[side], (r, side)                     # exactly the halo, ascending, nothing twice
            for q, a, b in p[side]:
                assert a < b and q != r and all(owner[z] == q for z in range(a, b))     # every plane from its owner
        for q, a, b in p["send"]:
            assert q != r and z0 <= a < b <= z1                     # only planes this rank owns
    sends = sorted((r, q, a, b) for r, p in enumerate(plans) for q, a, b in p["send"])
    recvs = sorted((q, r, a, b) for r, p in enumerate(plans) for side in ("lo", "hi") for q, a, b in p[side])
    assert sends == recvs                                           # every send has its receive and the other way round
    pairs = [(s, d) for s, d, _, _ in sends]
    assert len(pairs) == len(set(pairs))                            # at most one message per ordered pair: no tags needed
    if h == 0:
        assert not sends


def test_halo_plan_depth_and_empty_ranks():
    bounds = [shard_bounds(8, 3, r) for r in range(3)]              # 3 + 3 + 2 planes
    p = smooth.halo_plan(bounds, 2, 5)
    assert p["lo"] == [(0, 1, 3), (1, 3, 6)] and p["hi"] == [] and p["send"] == [(0, 6, 8), (1, 6, 8)]
    empty = smooth.halo_plan([shard_bounds(2, 3, r) for r in range(3)], 2, 4)
    assert empty == {"lo": [], "hi": [], "send": []}
    with pytest.raises(ValueError):
        smooth.halo_plan(bounds, 0, -1)


# ---------------------------------------------------------------------------------------------------------------- exchange_halos under gloo
H, W = 5, 6
CASES = {2: [(7, 2), (7, 9), (1, 3), (7, 0)], 3: [(8, 5), (2, 4), (8, 1)]}     # world -> (Z, h): deeper than a neighbour, a rank without planes


def _volume(Z):
    return torch.arange(Z * H * W, dtype=torch.int32).reshape(Z, H, W)         # every voxel holds its global index


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {}
        for i, (Z, h) in enumerate(CASES[world]):
            bounds = [shard_bounds(Z, world, r) for r in range(world)]
            z0, z1 = bounds[rank]
            lo, hi = smooth.exchange_halos(_volume(Z)[z0:z1].contiguous(), bounds, rank, None, h)
            assert lo.dtype == hi.dtype == torch.int32 and lo.shape[1:] == hi.shape[1:] == (H, W)
            res[f"lo{i}"], res[f"hi{i}"] = lo.numpy(), hi.numpy()
        np.savez(os.path.join(out_dir, f"out{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_exchange_halos_gloo(tmp_path, world):
    port = 33600 + (os.getpid() % 2000) + world
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        got = np.load(tmp_path / f"out{r}.npz")
        for i, (Z, h) in enumerate(CASES[world]):
            z0, z1 = shard_bounds(Z, world, r)
            vol = _volume(Z).numpy()
            lo = vol[max(z0 - h, 0):z0] if z1 > z0 else vol[:0]
            hi = vol[z1:min(z1 + h, Z)] if z1 > z0 else vol[:0]
            assert np.array_equal(got[f"lo{i}"], lo) and np.array_equal(got[f"hi{i}"], hi), (world, r, Z, h)


# ---------------------------------------------------------------------------------------------------------------- the scheme in numpy
@pytest.fixture(scope="module")
def whole():
    """the oracle on the whole volume, once per case"""
    cases = {name: ref.blob_case(name) for name in ("a", "b")}
    cases["sandwich"] = ref.sandwich()
    return {name: (vol, scale, saber_ref.fast_3d_gaussian_smoothing(vol, scale)) for name, (vol, scale) in cases.items()}


@pytest.mark.parametrize("name", ["a", "b", "sandwich"])
def test_restated_scheme_equals_the_oracle(whole, name):
    vol, scale, want = whole[name]
    Z = vol.shape[0]
    assert want.any()
    if name != "sandwich":
        assert vol.max() > 65535 and ((vol > 255) & (vol < 65536)).any()
    for parts in (1, 2, 3, Z):
        got = ref.smooth_chunks_ref(vol, ref.cuts_of(Z, parts), scale)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, parts)


def test_halo_deeper_than_every_chunk(whole):
    for name in ("a", "b"):
        vol, scale, _ = whole[name]
        counts = np.bincount(vol.ravel())
        h = max(ref.radius_of(c, scale) for c in counts[1:] if c)
        assert h > max(b - a for a, b in ref.cuts_of(vol.shape[0], 3))


def test_sandwich_needs_the_skip_rule(whole):
    vol, scale, want = whole["sandwich"]
    assert not vol[4].any() and int((want[4] == 7).sum()) == 304 and ref.radius_of(int((vol == 7).sum()), scale) == 8
    bounds = ref.cuts_of(9, 9)                                      # one-plane chunks: plane 4 owns no voxel of the label
    assert np.array_equal(ref.smooth_chunks_ref(vol, bounds, scale), want)
    naive = ref.smooth_chunks_ref(vol, bounds, scale, naive_skip=True)
    assert not np.array_equal(naive, want) and not naive[4].any()
