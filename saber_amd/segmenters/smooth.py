"""fast_3d_gaussian_smoothing (saber/filters/masks.py:230-287) with the label volume cut into consecutive z-chunks: every chunk is smoothed
on its own, from a few planes of its neighbours, and ends up with the uint8 bytes Engine.smooth_labels gives on the whole volume.

Why it is exact: a label's field is a separable zero-padded Gaussian of its 0/1 mask, with sigma from the label's voxel count in the WHOLE
volume and r = the tap radius.  An output voxel on plane z depends on the planes z - r .. z + r only.  With every label's whole-volume
count and h >= max r planes on either side (fewer where the volume ends) a chunk therefore holds everything its own planes depend on, and
the kernels sum an output's taps in the same order as on the whole volume (csrc/smooth3d.hip: saber_smooth_labels_chunk).

Per chunk (one rank of segment_volume_sharded, or one entry of smooth_labels_chunks):
  1. count      largest label value and the dense count table of the own planes (Engine.label_max / label_counts)
  2. reduce     maximum of the label values, then sum of the tables, over all chunks: the whole volume's counts
  3. radius     h = the library's radius of the largest count (Engine.smooth_radius; the radius grows with the count)
  4. halos      the planes [z0 - h, z0) and [z1, z1 + h), clipped to the volume, from the chunks that own them (halo_plan, exchange_halos)
  5. smooth     one Engine.smooth_labels_chunk call on (lower halo, own planes, upper halo): three buffers, nothing is concatenated
"""
from typing import List, Sequence, Tuple

import numpy as np
import torch

MAX_LABEL = 1 << 22        # SM_MAX_LABEL of csrc/smooth3d.hip


# ---------------------------------------------------------------------------------------------------------------- the plan (pure Python)
def _wanted(bounds, q: int, h: int, Z: int):
    """the two plane ranges rank q needs beside its own: below and above (empty for a rank that owns nothing)"""
    z0, z1 = bounds[q]
    if z1 <= z0:
        return (z0, z0), (z1, z1)
    return (max(z0 - h, 0), z0), (z1, min(z1 + h, Z))


def _cut(rng, bounds, skip: int):
    """the pieces of the plane range `rng` by owner: [(owner, a, b)], ascending"""
    out = []
    for p, (a, b) in enumerate(bounds):
        lo, hi = max(a, rng[0]), min(b, rng[1])
        if p != skip and lo < hi:
            out.append((p, lo, hi))
    return sorted(out, key=lambda t: t[1])


def halo_plan(bounds, rank: int, h: int) -> dict:
    """Who hands which planes to whom for halos of depth h.  bounds[q] = (z0, z1) of rank q, consecutive in z.  Returns
    {"lo": [(owner, a, b)], "hi": [(owner, a, b)], "send": [(receiver, a, b)]}: the global plane ranges [a, b) `rank` receives for the
    planes below and above its own (ascending: concatenated they are [z0 - h, z0) and [z1, z1 + h) clipped to the volume) and the
    ranges of its own planes it sends.  A halo deeper than a neighbour comes from several owners; a rank that owns nothing receives
    nothing and sends nothing.  Between two ranks at most one range travels in either direction."""
    h = int(h)
    if h < 0:
        raise ValueError(f"halo_plan: halo depth {h}")
    Z = max([b for _, b in bounds] + [0])
    below, above = _wanted(bounds, rank, h, Z)
    send = []
    for q in range(len(bounds)):
        if q == rank:
            continue
        for rng in _wanted(bounds, q, h, Z):
            send += [(q, a, b) for p, a, b in _cut(rng, bounds, q) if p == rank]
    return {"lo": _cut(below, bounds, rank), "hi": _cut(above, bounds, rank), "send": sorted(send)}


def _peer(dist, group, q: int) -> int:
    return dist.get_global_rank(group, q) if group is not None else q


def exchange_halos(labels: torch.Tensor, bounds, rank: int, group, h: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The planes below and above this rank's chunk, point to point: a rank receives only the planes of halo_plan.  labels: this rank's
    (z1 - z0, H, W) planes (0 planes for a rank that owns nothing).  Returns (lo, hi) on the chunk's device, in its dtype.  The planes
    travel as bytes (gloo has no 16-bit types; RCCL moves the same bytes); device tensors under a host backend are staged through
    host memory, as stitch._all_gather_bytes does."""
    import torch.distributed as dist
    plan = halo_plan(bounds, rank, h)
    z0 = bounds[rank][0]
    shape = tuple(int(v) for v in labels.shape[1:])
    staged = labels.is_cuda and dist.get_backend(group) != "nccl"
    wire = torch.device("cpu") if staged else labels.device
    ops, parts = [], {"lo": [], "hi": []}
    for q, a, b in plan["send"]:
        piece = labels[a - z0: b - z0].contiguous().view(torch.uint8)
        ops.append(dist.P2POp(dist.isend, piece.cpu() if staged else piece, _peer(dist, group, q), group))
    for side in ("lo", "hi"):
        for q, a, b in plan[side]:
            buf = torch.empty((b - a,) + shape, dtype=labels.dtype, device=wire)
            parts[side].append(buf)
            ops.append(dist.P2POp(dist.irecv, buf.view(torch.uint8), _peer(dist, group, q), group))
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    empty = torch.empty((0,) + shape, dtype=labels.dtype, device=labels.device)
    return tuple(torch.cat(parts[side], 0).to(labels.device) if parts[side] else empty for side in ("lo", "hi"))


# ---------------------------------------------------------------------------------------------------------------- the steps of one chunk
def _max_of(engine, labels) -> int:
    """step 1, first half: the largest label value of the own planes"""
    return engine.label_max(labels) if labels.shape[0] else 0


def _counts_of(engine, labels, n: int) -> torch.Tensor:
    """step 1, second half (the whole volume's maximum is known): the (n,) int64 count table of the own planes"""
    if labels.shape[0]:
        return engine.label_counts(labels, n)
    return torch.zeros((n,), dtype=torch.int64, device=engine.device)


def _table(engine, counts: np.ndarray, scale: float):
    """the whole volume's count table -> (ids ascending, their counts, halo depth)"""
    ids = np.flatnonzero(counts[1:]) + 1
    cnt = counts[ids].astype(np.int64)
    return ids, cnt, (engine.smooth_radius(int(cnt.max()), scale) if ids.size else 0)


def _check_max(who: str, m: int):
    if m > MAX_LABEL:
        raise ValueError(f"{who}: label values above 2^22 are not supported")


def smooth_labels_chunks(engine, chunks: Sequence[torch.Tensor], scale: float) -> List[torch.Tensor]:
    """Engine.smooth_labels of one volume handed over as consecutive z-chunks, in one process.  chunks: (Zc,H,W) label tensors of one
    dtype on the engine's device, in z order (Zc = 0 is allowed).  Returns the chunks' (Zc,H,W) uint8 results.  The steps are those of
    smooth_rank, with the reduction and the halo exchange done in process (the halos are slices of the neighbours)."""
    who = "smooth_labels_chunks"
    if len(chunks) == 0:
        raise ValueError(f"{who}: no chunks")
    if any(not isinstance(c, torch.Tensor) or c.dim() != 3 for c in chunks):
        raise ValueError(f"{who}: every chunk must be a (Zc,H,W) tensor")
    H, W = (int(v) for v in chunks[0].shape[1:])
    if any(tuple(int(v) for v in c.shape[1:]) != (H, W) for c in chunks):
        raise ValueError(f"{who}: every chunk must be (Zc,H,W) with the same H and W")
    if any(c.dtype != chunks[0].dtype for c in chunks):
        raise ValueError(f"{who}: every chunk must have the same dtype")
    chunks = [c.contiguous() for c in chunks]
    cuts = np.concatenate([[0], np.cumsum([int(c.shape[0]) for c in chunks])])
    bounds = [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    Z = bounds[-1][1]
    m = max(_max_of(engine, c) for c in chunks)
    _check_max(who, m)
    empty = lambda c: torch.zeros(tuple(c.shape), dtype=torch.uint8, device=engine.device)
    if m == 0:
        return [empty(c) for c in chunks]
    counts = sum(_counts_of(engine, c, m + 1) for c in chunks).cpu().numpy()
    ids, cnt, h = _table(engine, counts, scale)
    out = []
    for i, c in enumerate(chunks):
        if c.shape[0] == 0:
            out.append(empty(c))
            continue
        plan = halo_plan(bounds, i, h)
        halo = {side: [chunks[q][a - bounds[q][0]: b - bounds[q][0]] for q, a, b in plan[side]] for side in ("lo", "hi")}
        # planes of one neighbour are a view of it; only a halo that spans several chunks is copied together
        lo, hi = (None if not halo[side] else halo[side][0] if len(halo[side]) == 1 else torch.cat(halo[side], 0) for side in ("lo", "hi"))
        z0, z1 = bounds[i]
        n_lo, n_hi = (0 if t is None else int(t.shape[0]) for t in (lo, hi))
        out.append(engine.smooth_labels_chunk(c, lo, hi, ids, cnt, scale, z0 - n_lo == 0, z1 + n_hi == Z)[0])
    return out


# ---------------------------------------------------------------------------------------------------------------- one rank of a process group
def _all_reduce(dist, t: torch.Tensor, op, group) -> torch.Tensor:
    """all_reduce of an int64 tensor; a device tensor under a host backend is staged through host memory"""
    if t.is_cuda and dist.get_backend(group) != "nccl":
        host = t.cpu()
        dist.all_reduce(host, op=op, group=group)
        return host
    dist.all_reduce(t, op=op, group=group)
    return t


def smooth_rank(engine, labels: torch.Tensor, Z: int, H: int, W: int, bounds, rank: int, group, scale: float, stamp=None) -> torch.Tensor:
    """One rank's part of the sharded smoothing.  labels: this rank's (z1 - z0, H, W) label planes on the engine's device (what stitch_rank
    returned); bounds[q] = (z0, z1) of rank q.  Returns this rank's (z1 - z0, H, W) uint8 chunk of Engine.smooth_labels on the whole
    volume.  Collectives, in this order on every rank: all-reduce (max) of the largest label value, all-reduce (sum) of the int64 count
    table, the point-to-point halo exchange.  stamp: called with "counted" and "halos" when those steps are done."""
    import torch.distributed as dist
    world = len(bounds)
    z0, z1 = bounds[rank]
    labels = labels.contiguous()
    m = _max_of(engine, labels)
    if world > 1:
        m = int(_all_reduce(dist, torch.tensor([m], dtype=torch.int64, device=labels.device), dist.ReduceOp.MAX, group).item())
    _check_max("sharded smoothing", m)
    out_empty = lambda: torch.zeros((z1 - z0, H, W), dtype=torch.uint8, device=labels.device)
    if m == 0:                                          # the same on every rank: nobody waits for anybody
        for key in ("counted", "halos") if stamp else ():
            stamp(key)
        return out_empty()
    counts = _counts_of(engine, labels, m + 1)
    if world > 1:
        counts = _all_reduce(dist, counts, dist.ReduceOp.SUM, group)
    ids, cnt, h = _table(engine, counts.cpu().numpy(), scale)
    if stamp:
        stamp("counted")
    lo = hi = None
    if world > 1:
        lo, hi = exchange_halos(labels, bounds, rank, group, h)
    if stamp:
        stamp("halos")
    if z1 == z0:
        return out_empty()
    n_lo, n_hi = (0 if t is None else int(t.shape[0]) for t in (lo, hi))
    return engine.smooth_labels_chunk(labels, lo, hi, ids, cnt, scale, z0 - n_lo == 0, z1 + n_hi == Z)[0]


def gather_smoothed(chunk: torch.Tensor, Z: int, H: int, W: int, bounds, rank: int, group, gather: str):
    """The uint8 chunks of every rank as one (Z,H,W) tensor on every rank (gather="all") or on rank 0 (gather="rank0": None elsewhere):
    1 B per voxel, a quarter of what stitch.gather_labels moves."""
    import torch.distributed as dist
    from .stitch import _all_gather_bytes
    world = len(bounds)
    if world == 1:
        return chunk
    depth = max(b - a for a, b in bounds)
    pad = torch.zeros((depth, H, W), dtype=torch.uint8, device=chunk.device)
    pad[:chunk.shape[0]] = chunk
    if gather == "all":
        full = torch.empty((world * depth, H, W), dtype=torch.uint8, device=chunk.device)
        _all_gather_bytes(dist, full, pad, group)
    else:
        staged = pad.is_cuda and dist.get_backend(group) != "nccl"
        src = pad.cpu() if staged else pad
        parts = [torch.empty_like(src) for _ in range(world)] if rank == 0 else None
        dist.gather(src, parts, dst=_peer(dist, group, 0), group=group)
        if rank != 0:
            return None
        full = torch.cat(parts, 0).to(chunk.device)
    return torch.cat([full[q * depth: q * depth + (b - a)] for q, (a, b) in enumerate(bounds)], 0)
