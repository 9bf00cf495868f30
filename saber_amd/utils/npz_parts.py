"""Fixture archives in parts: every file under tests/golden/ stays below 1 MiB.

`save(path, arrays)` writes np.savez_compressed(path, **arrays) when the archive fits; otherwise it writes <stem>.part<k>.npz files that
each fit, an array too large for one part split along its first axis into pieces named <key>@<i>.  `load(path)` returns the same
{key: array} either way (pieces concatenated back in order, bit for bit), so callers keep naming the archive by its logical path."""
import glob
import os
import re
import zlib

import numpy as np

LIMIT = 1 << 20          # bytes per committed file
_BUDGET = 900_000        # deflated bytes per part: headroom for the zip and .npy headers below LIMIT


def _stem(path):
    return path[:-4] if path.endswith(".npz") else path


def part_paths(path):
    """The <stem>.part<k>.npz files of `path`, in part order (empty when the archive is one file)."""
    found = []
    for p in glob.glob(glob.escape(_stem(path)) + ".part*.npz"):
        m = re.search(r"\.part(\d+)\.npz$", p)
        if m:
            found.append((int(m.group(1)), p))
    return [p for _, p in sorted(found)]


def exists(path):
    return os.path.exists(path) or bool(part_paths(path))


def load(path):
    """{key: array} of the archive `path`, whole or in parts."""
    if os.path.exists(path):
        with np.load(path, allow_pickle=False) as Z:
            return {k: Z[k] for k in Z.files}
    parts = part_paths(path)
    if not parts:
        raise FileNotFoundError(path)
    out, pieces = {}, {}
    for p in parts:
        with np.load(p, allow_pickle=False) as Z:
            for k in Z.files:
                name, sep, i = k.rpartition("@")
                if sep and i.isdigit():
                    out.setdefault(name, None)
                    pieces.setdefault(name, []).append((int(i), Z[k]))
                else:
                    out[k] = Z[k]
    for name, got in pieces.items():
        out[name] = np.concatenate([a for _, a in sorted(got, key=lambda t: t[0])], axis=0)
    return out


def _deflated(a):
    return len(zlib.compress(np.ascontiguousarray(a).tobytes()))


def save(path, arrays):
    """Write `arrays` as the archive `path` (one file or parts, see the module docstring); returns the files written."""
    for p in part_paths(path) + ([path] if os.path.exists(path) else []):
        os.remove(p)
    pieces = []
    for k, a in arrays.items():
        a = np.asarray(a)
        n = _deflated(a)
        if n <= _BUDGET or a.ndim == 0:
            pieces.append((k, a, n))
            continue
        c = -(-n // _BUDGET)
        while True:
            chunks = np.array_split(a, c, axis=0)
            sizes = [_deflated(x) for x in chunks]
            if max(sizes) <= _BUDGET or c >= a.shape[0]:
                break
            c += 1
        pieces += [(f"{k}@{i}", x, s) for i, (x, s) in enumerate(zip(chunks, sizes))]
    if sum(n for _, _, n in pieces) <= _BUDGET:
        groups = [pieces]
        names = [path]
    else:
        groups, cur, tot = [], [], 0
        for pc in pieces:
            if cur and tot + pc[2] > _BUDGET:
                groups.append(cur)
                cur, tot = [], 0
            cur.append(pc)
            tot += pc[2]
        groups.append(cur)
        names = [f"{_stem(path)}.part{i}.npz" for i in range(len(groups))]
    for name, g in zip(names, groups):
        np.savez_compressed(name, **{k: a for k, a, _ in g})
        if os.path.getsize(name) >= LIMIT:
            raise ValueError(f"{name}: {os.path.getsize(name)} bytes, not below {LIMIT}")
    return names
