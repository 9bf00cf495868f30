"""The 3-D stitch (utils.separate_masks, saber/segmenters/utils.py:88-131) with the volume cut into consecutive z-chunks: every chunk is
labelled on its own, only what touches a seam between two chunks is exchanged, and every chunk ends up with the final uint32 labels of
its planes - bit for bit what separate_masks gives on the whole volume.

Why it is exact: the labelling core (csrc/ccl.h) makes a component's root its first voxel in C-order scan, and z-chunks are contiguous in
that order.  root + z0*H*W is therefore a global voxel index, a component that spans chunks has the minimum of its pieces' roots as its
global first voxel, and scipy.ndimage.label's numbering is the rank of those minima among the components that survive the size filter.

Per chunk (one rank of segment_volume_sharded, or one entry of separate_masks_chunks):
  1. label      init / merge / flatten / count on the chunk alone (Engine.cc_chunk_label; label_chunk_host for CPU planes)
  2. seam       the chunk receives the root plane the next non-empty chunk's first plane holds; the roots that touch across the seam come
                from Engine.cc_seam_pairs (seam_pairs_host)
  3. record     the roots on a plane that faces a neighbour (global ids), their sizes, the pair list: exchanged among all chunks
  4. resolve    resolve_seams - host, numpy, the same on every rank: components of the seam graph, their minimum node and total size
  5. own        roots that touch no seam are kept by their own size (Engine.cc_chunk_roots); a chunk owns those and the kept seam components
                whose minimum lies in its index range; their ascending order gives each a position, their number is the chunk's count
  6. ids        second exchange: count and (minimum, position) of the owned seam components; id = sum of the counts before + position + 1
  7. finish     the owned roots and every seam root get their ids (0 = dropped), the chunk is relabelled (Engine.cc_chunk_finish)
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

NONE = 0xFFFFFFFF          # background in `lab` (CCL_NONE of csrc/ccl.h)
_E = np.zeros(0, dtype=np.int64)


def min_voxels_of(min_mask_area: int) -> int:
    """The size filter of separate_masks as one threshold: components below min_mask_area * 10 voxels go when that product exceeds 1."""
    return max(int(min_mask_area) * 10, 1)


# ---------------------------------------------------------------------------------------------------------------- host pieces
def resolve_seams(nodes, sizes, pairs, min_voxels: int):
    """Joins the chunks' roots across the seams.  nodes: the global ids of the roots that face a seam (each once), sizes: their voxel
    counts inside their own chunk, pairs: (k,2) rows of node ids that touch (repeats allowed).  Returns, aligned with `nodes`:
    rep (the minimum node of the node's seam component = the component's global first voxel), total (the component's voxels) and keep
    (total >= max(min_voxels, 1)).  Pure function of its arguments as sets: the order of nodes and pairs does not matter."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if nodes.size != sizes.size:
        raise ValueError(f"resolve_seams: {nodes.size} nodes and {sizes.size} sizes")
    m = nodes.size
    if m == 0:
        if pairs.size:
            raise ValueError("resolve_seams: pairs without nodes")
        return _E.copy(), _E.copy(), np.zeros(0, dtype=bool)
    order = np.argsort(nodes, kind="stable")
    sn = nodes[order]
    if np.any(sn[1:] == sn[:-1]):
        raise ValueError("resolve_seams: a node is listed twice")
    idx = np.minimum(np.searchsorted(sn, pairs), m - 1)
    if np.any(sn[idx] != pairs):
        raise ValueError("resolve_seams: a pair names a root that is not a node")
    graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (idx[:, 0], idx[:, 1])), shape=(m, m))
    ncomp, comp = connected_components(graph, directed=False)
    rep_c = np.full(ncomp, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(rep_c, comp, sn)
    tot_c = np.zeros(ncomp, dtype=np.int64)
    np.add.at(tot_c, comp, sizes[order])
    rep, total = np.empty(m, dtype=np.int64), np.empty(m, dtype=np.int64)
    rep[order], total[order] = rep_c[comp], tot_c[comp]
    return rep, total, total >= max(int(min_voxels), 1)


def label_chunk_host(planes):
    """Engine.cc_chunk_label on the host (scipy): planes (Z,H,W), foreground = non-zero.  Returns (lab, sizes), (Z,H,W) uint32:
    lab[v] = flat index of the first voxel of v's 26-connected component inside the chunk (NONE for background), sizes[root] = its voxels."""
    from scipy import ndimage as ndi
    fg = np.ascontiguousarray(np.asarray(planes) != 0)
    lab_s, k = ndi.label(fg, structure=np.ones((3, 3, 3), dtype=bool))
    flat = lab_s.ravel()
    first = np.full(k + 1, NONE, dtype=np.uint32)
    if k:
        vals, where = np.unique(flat, return_index=True)           # first occurrence of 0 (if any) and of every label
        first[vals] = where.astype(np.uint32)
        first[0] = NONE
    lab = first[flat].reshape(fg.shape)
    sizes = np.zeros(fg.size, dtype=np.uint32)
    if k:
        sizes[first[1:]] = np.bincount(flat, minlength=k + 1)[1:].astype(np.uint32)
    return lab, sizes.reshape(fg.shape)


def seam_pairs_host(a_roots, b_roots, a_offset: int = 0, b_offset: int = 0) -> np.ndarray:
    """Engine.cc_seam_pairs on the host: the unique sorted rows (root in a + a_offset, root in b + b_offset) of what touches across the
    seam, under the labelling's merge rule (per row offset the centre neighbour if it is foreground, else the two diagonals)."""
    a, b = np.asarray(a_roots, dtype=np.uint32), np.asarray(b_roots, dtype=np.uint32)
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError(f"seam_pairs_host: planes of shapes {a.shape} and {b.shape}")
    H, W = a.shape
    bp = np.full((H + 2, W + 2), NONE, dtype=np.uint32)
    bp[1:-1, 1:-1] = b
    fg = a != NONE
    rows = []
    for dy in (-1, 0, 1):
        r = bp[1 + dy: 1 + dy + H]
        left, centre, right = r[:, :-2], r[:, 1:-1], r[:, 2:]
        c = fg & (centre != NONE)
        rows.append(np.stack([a[c], centre[c]], 1))
        for side in (left, right):
            d = fg & (centre == NONE) & (side != NONE)
            rows.append(np.stack([a[d], side[d]], 1))
    out = np.concatenate(rows).astype(np.int64)
    if out.size == 0:
        return out.reshape(0, 2)
    out += np.array([int(a_offset), int(b_offset)], dtype=np.int64)
    return np.unique(out, axis=0)


class _HostOps:
    """the chunk steps on numpy arrays (CPU planes: the host route of the driver)"""

    def label(self, planes):
        return label_chunk_host(planes.numpy() if isinstance(planes, torch.Tensor) else planes)

    def plane(self, lab, i):
        return lab[i]

    def face_nodes(self, lab, sizes, planes_idx):
        roots = np.unique(lab[planes_idx])
        roots = roots[roots != NONE].astype(np.int64)
        return roots, sizes.reshape(-1)[roots].astype(np.int64)

    def seam_pairs(self, a, a_off, b, b_off):
        return seam_pairs_host(a, b, a_off, b_off)

    def chunk_roots(self, lab, sizes, min_voxels, exclude):
        flat, sz = lab.reshape(-1), sizes.reshape(-1)
        roots = np.flatnonzero(flat == np.arange(flat.size, dtype=np.uint32))
        ok = sz[roots] >= max(int(min_voxels), 1)
        ok &= ~np.isin(roots, exclude)
        return roots[ok].astype(np.int64)

    def finish(self, lab, sizes, roots, ids):
        table = np.zeros(lab.size + 1, dtype=np.uint32)             # the extra entry takes the background
        table[np.asarray(roots, dtype=np.int64)] = np.asarray(ids, dtype=np.uint32)
        return table[np.minimum(lab, lab.size)]

    def empty(self, H, W):
        return np.zeros((0, H, W), dtype=np.uint32)


class _DeviceOps:
    """the chunk steps on the engine's device (csrc/cc3d.hip)"""

    def __init__(self, engine):
        self.engine = engine

    def label(self, planes):
        return self.engine.cc_chunk_label(planes.contiguous())

    def plane(self, lab, i):
        return lab[i]

    def face_nodes(self, lab, sizes, planes_idx):
        roots = torch.unique(lab[planes_idx])
        roots = roots[roots >= 0].long()
        return roots.cpu().numpy(), sizes.view(-1)[roots].cpu().numpy().astype(np.int64)

    def seam_pairs(self, a, a_off, b, b_off):
        return self.engine.cc_seam_pairs(a.contiguous(), b.contiguous(), a_off, b_off)

    def chunk_roots(self, lab, sizes, min_voxels, exclude):
        return self.engine.cc_chunk_roots(lab, sizes, min_voxels, exclude)

    def finish(self, lab, sizes, roots, ids):
        return self.engine.cc_chunk_finish(lab, sizes, roots, ids)

    def empty(self, H, W):
        return torch.zeros((0, H, W), dtype=torch.int32, device=self.engine.device)


# ---------------------------------------------------------------------------------------------------------------- the phases of one chunk
class _Chunk:
    """one chunk between its labelling and its relabelling; z0 .. z0 + Zc of a volume of H x W planes"""

    def __init__(self, ops, planes, z0: int, H: int, W: int):
        self.ops, self.z0, self.Zc, self.H, self.W = ops, int(z0), int(planes.shape[0]) if planes is not None else 0, H, W
        self.off = self.z0 * H * W
        self.lab = self.sizes = None
        self.seam_local = _E
        if self.Zc:
            self.lab, self.sizes = ops.label(planes)

    def first_plane(self):
        return self.ops.plane(self.lab, 0)

    def record(self, has_prev: bool, next_plane=None, next_off: int = 0):
        """(nodes, sizes, pairs) of this chunk: the global ids of the roots on a plane that faces a neighbour, their sizes, and the
        pairs across the seam to the next non-empty chunk (whose first root plane is next_plane)."""
        if not self.Zc:
            return _E, _E, _E.reshape(0, 2)
        faces = sorted(set(([0] if has_prev else []) + ([self.Zc - 1] if next_plane is not None else [])))
        sz = _E
        if faces:
            self.seam_local, sz = self.ops.face_nodes(self.lab, self.sizes, faces)
        pairs = _E.reshape(0, 2)
        if next_plane is not None:
            pairs = self.ops.seam_pairs(self.ops.plane(self.lab, self.Zc - 1), self.off, next_plane, next_off)
        return self.seam_local + self.off, sz, pairs

    def own(self, resolved, min_voxels: int):
        """(count, owned seam components' minima, their positions): what this chunk numbers."""
        if not self.Zc:
            return 0, _E, _E
        nodes, rep, keep = resolved
        self.kept_local = self.ops.chunk_roots(self.lab, self.sizes, min_voxels, self.seam_local)
        reps = np.unique(rep[keep])
        owned = reps[(reps >= self.off) & (reps < self.off + self.Zc * self.H * self.W)]
        merged = np.sort(np.concatenate([self.kept_local + self.off, owned]))
        self.kept_pos = np.searchsorted(merged, self.kept_local + self.off)
        return int(merged.size), owned, np.searchsorted(merged, owned)

    def finish(self, resolved, owned_all, prefix: int):
        """the chunk's labels, given every rank's (count, owned, positions) as the cumulative `prefix` of this chunk and the (minimum, id)
        table of all kept seam components"""
        if not self.Zc:
            return self.ops.empty(self.H, self.W)
        nodes, rep, keep = resolved
        reps, rep_ids = owned_all
        mine = np.searchsorted(nodes, self.seam_local + self.off)
        seam_ids = np.zeros(self.seam_local.size, dtype=np.int64)
        k = keep[mine] if mine.size else np.zeros(0, dtype=bool)
        seam_ids[k] = rep_ids[np.searchsorted(reps, rep[mine][k])]
        roots = np.concatenate([self.kept_local, self.seam_local])
        ids = np.concatenate([prefix + self.kept_pos + 1, seam_ids])
        return self.ops.finish(self.lab, self.sizes, roots, ids)


def _resolve_records(records, min_voxels: int):
    """every chunk's record -> (nodes ascending, rep, keep)"""
    nodes = np.concatenate([np.asarray(r[0], dtype=np.int64) for r in records] + [_E])
    sizes = np.concatenate([np.asarray(r[1], dtype=np.int64) for r in records] + [_E])
    pairs = np.concatenate([np.asarray(r[2], dtype=np.int64).reshape(-1, 2) for r in records] + [_E.reshape(0, 2)])
    rep, _, keep = resolve_seams(nodes, sizes, pairs, min_voxels)
    order = np.argsort(nodes, kind="stable")
    return nodes[order], rep[order], keep[order]


def _id_table(owns):
    """every chunk's (count, owned, positions) -> (prefix per chunk, (minima ascending, ids), total)"""
    counts = np.array([o[0] for o in owns], dtype=np.int64)
    prefix = np.concatenate([[0], np.cumsum(counts)])
    reps = np.concatenate([np.asarray(o[1], dtype=np.int64) for o in owns] + [_E])
    ids = np.concatenate([prefix[q] + np.asarray(o[2], dtype=np.int64) + 1 for q, o in enumerate(owns)] + [_E])
    order = np.argsort(reps, kind="stable")
    return prefix, (reps[order], ids[order]), int(prefix[-1])


def _check_volume(who: str, Z: int, H: int, W: int):
    if Z * H * W >= 0x7FFFFFFF:
        raise ValueError(f"{who}: volumes of 2^31 - 1 voxels or more are not supported (a global voxel index must fit 32 bits)")


def separate_masks_chunks(engine, chunks: Sequence, min_mask_area: int = 100) -> Tuple[List, int]:
    """separate_masks of one volume handed over as consecutive z-chunks, in one process.  chunks: (Zc,H,W) uint16 / int16 tensors on the
    engine's device, in z order (Zc = 0 is allowed); with engine=None, CPU tensors or numpy arrays on the host route.  Returns (the
    chunks' labels - int32 device tensors holding uint32, or uint32 arrays on the host route - and the number of labels).  The phases
    and the resolve are those of the sharded driver, with the exchange done in process."""
    if len(chunks) == 0:
        raise ValueError("separate_masks_chunks: no chunks")
    ops = _DeviceOps(engine) if engine is not None else _HostOps()
    H, W = (int(v) for v in chunks[0].shape[1:])
    if any(c.ndim != 3 or tuple(int(v) for v in c.shape[1:]) != (H, W) for c in chunks):
        raise ValueError("separate_masks_chunks: every chunk must be (Zc,H,W) with the same H and W")
    bounds = np.concatenate([[0], np.cumsum([int(c.shape[0]) for c in chunks])])
    _check_volume("separate_masks_chunks", int(bounds[-1]), H, W)
    min_voxels = min_voxels_of(min_mask_area)
    states = [_Chunk(ops, c if c.shape[0] else None, bounds[i], H, W) for i, c in enumerate(chunks)]
    live = [i for i, s in enumerate(states) if s.Zc]
    nxt = {a: b for a, b in zip(live[:-1], live[1:])}
    records = []
    for i, s in enumerate(states):
        n = states[nxt[i]] if i in nxt else None
        records.append(s.record(bool(live) and s.Zc > 0 and i != live[0], n.first_plane() if n else None, n.off if n else 0))
    resolved = _resolve_records(records, min_voxels)
    owns = [s.own(resolved, min_voxels) for s in states]
    prefix, table, total = _id_table(owns)
    return [s.finish(resolved, table, int(prefix[i])) for i, s in enumerate(states)], total


# ---------------------------------------------------------------------------------------------------------------- one rank of a process group
def _all_gather_bytes(dist, out: torch.Tensor, mine: torch.Tensor, group):
    """all_gather_into_tensor on byte views (gloo has no 16-bit collectives; RCCL moves the same bytes); device tensors under a host
    backend are staged through host memory, as the plane gather of segment_volume_sharded is"""
    out_b = out.view(torch.uint8).flatten()             # the concatenated form: gloo takes no stacked output
    mine_b = mine.contiguous().view(torch.uint8).flatten()
    if mine.is_cuda and dist.get_backend(group) != "nccl":
        host = torch.empty(out_b.shape, dtype=torch.uint8)
        dist.all_gather_into_tensor(host, mine_b.cpu(), group=group)
        out_b.copy_(host)
    else:
        dist.all_gather_into_tensor(out_b, mine_b, group=group)


def stitch_rank(engine, planes, Z: int, H: int, W: int, bounds, rank: int, group, min_mask_area: int, stamp=None):
    """One rank's part of the sharded stitch.  planes: this rank's (z1 - z0, H, W) label planes (a device tensor with `engine`, else a CPU
    tensor: host route); bounds[q] = (z0, z1) of rank q.  Returns (the chunk's labels, number of labels in the whole volume).
    Collectives, in this order on every rank: all-gather of the first root planes (H*W*4 bytes each), all_gather_object of the seam
    records, all_gather_object of the counts and owned seam components."""
    import torch.distributed as dist
    _check_volume("sharded stitch", Z, H, W)
    world = len(bounds)
    ops = _DeviceOps(engine) if engine is not None else _HostOps()
    z0, z1 = bounds[rank]
    min_voxels = min_voxels_of(min_mask_area)
    me = _Chunk(ops, planes if z1 > z0 else None, z0, H, W)
    live = [q for q in range(world) if bounds[q][1] > bounds[q][0]]
    after = [q for q in live if q > rank]
    nxt = after[0] if me.Zc and after else None
    next_plane = None
    if world > 1:
        dev = planes.device if isinstance(planes, torch.Tensor) else torch.device("cpu")
        if me.Zc:
            first = me.first_plane()
            first = first if isinstance(first, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(first).view(np.int32))
        else:
            first = torch.full((H, W), -1, dtype=torch.int32, device=dev)
        firsts = torch.empty((world, H, W), dtype=torch.int32, device=first.device)
        _all_gather_bytes(dist, firsts, first, group)
        if nxt is not None:
            next_plane = firsts[nxt] if engine is not None else firsts[nxt].numpy().view(np.uint32)
    record = me.record(me.Zc > 0 and rank != live[0], next_plane, bounds[nxt][0] * H * W if nxt is not None else 0)
    if stamp:
        stamp("labelled")
    records = [record]
    if world > 1:
        records = [None] * world
        dist.all_gather_object(records, record, group=group)
    resolved = _resolve_records(records, min_voxels)
    own = me.own(resolved, min_voxels)
    owns = [own]
    if world > 1:
        owns = [None] * world
        dist.all_gather_object(owns, own, group=group)
    prefix, table, total = _id_table(owns)
    if stamp:
        stamp("resolved")
    return me.finish(resolved, table, int(prefix[rank])), total


def gather_labels(labels, Z: int, H: int, W: int, bounds, rank: int, group, gather: str):
    """The label chunks of every rank as one (Z,H,W) tensor on every rank (gather="all") or on rank 0 (gather="rank0": None elsewhere).
    labels: this rank's chunk (int32 tensor holding uint32, or a uint32 array).  Returns an int32 tensor on the chunk's device."""
    import torch.distributed as dist
    world = len(bounds)
    t = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(labels.view(np.int32))
    if world == 1:
        return t
    chunk = max(b - a for a, b in bounds)
    pad = torch.zeros((chunk, H, W), dtype=torch.int32, device=t.device)
    pad[:t.shape[0]] = t
    staged = pad.is_cuda and dist.get_backend(group) != "nccl"
    if gather == "all":
        full = torch.empty((world * chunk, H, W), dtype=torch.int32, device=t.device)
        _all_gather_bytes(dist, full, pad, group)
    else:
        src = pad.cpu() if staged else pad
        parts = [torch.empty_like(src) for _ in range(world)] if rank == 0 else None
        dist.gather(src, parts, dst=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        if rank != 0:
            return None
        full = torch.cat(parts, 0).to(t.device)
    return torch.cat([full[q * chunk: q * chunk + (b - a)] for q, (a, b) in enumerate(bounds)], 0)
