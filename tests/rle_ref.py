"""Host restatement of the uncompressed run-length encoding of masks, written from its definition: the mask is flattened in column-major
order (pixel (y, x) has position x H + y); `counts` alternates runs of zeros and ones, starts with a zeros run (0 when pixel (0,0) is
set) and sums to H W.  Plus the bit packing of the mask generator's rows (bit b of word w of a row = pixel 32 w + b) and the stacks of
constructed masks the CPU and GPU tests share."""
import numpy as np


def pack_bits(masks, padding=False):
    """(n,H,W) bool -> (n,H,ceil(W/32)) uint32; padding=True sets the bits beyond W in every row's last word"""
    n, H, W = masks.shape
    W32 = (W + 31) // 32
    padded = np.zeros((n, H, W32 * 32), dtype=np.uint8)
    padded[..., :W] = masks
    if padding:
        padded[..., W:] = 1
    return np.packbits(padded, axis=-1, bitorder="little").view(np.uint32).reshape(n, H, W32)


def unpack_bits(words, W):
    n, H, W32 = words.shape
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(n, H, W32 * 4), axis=-1, bitorder="little")[..., :W].astype(bool)


def encode(mask):
    """(H,W) bool -> list of run lengths"""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)                # column-major
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1               # positions where a new run starts
    bounds = np.concatenate([[0], change, [flat.size]])
    counts = np.diff(bounds).tolist()
    return ([0] + counts) if flat[0] else counts


def decode(counts, H, W):
    """run lengths -> (H,W) bool; runs are clamped at H W and pixels behind the last run are zero"""
    flat = np.zeros(H * W, dtype=bool)
    pos = 0
    for k, c in enumerate(counts):
        if k & 1:
            flat[min(pos, H * W):min(pos + int(c), H * W)] = True
        pos += int(c)
    return flat.reshape(W, H).T


def encode_stack(masks):
    """(n,H,W) bool -> (counts uint32 (total,), offsets int64 (n + 1,))"""
    lists = [encode(m) for m in masks]
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(c) for c in lists])
    return np.concatenate([np.asarray(c, dtype=np.uint32) for c in lists]), offsets


SIZES = [(1, 1), (1, 70), (70, 1), (64, 32), (65, 33), (130, 95)]


def constructed_stack(H, W, seed=0):
    """(names, (n,H,W) bool): the masks of the issue's list at one size, an empty mask between two dense ones"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[:H, :W]
    z = np.zeros((H, W), bool)
    out = []

    def add(name, m):
        out.append((name, np.ascontiguousarray(m, dtype=bool)))

    add("checkerboard 0", (yy + xx) % 2 == 0)
    add("empty", z)
    add("checkerboard 1", (yy + xx) % 2 == 1)
    add("full", ~z)
    first, last = z.copy(), z.copy()
    first[0, 0] = True
    last[H - 1, W - 1] = True
    add("first pixel", first)
    add("last pixel", last)
    add("vertical stripes", xx % 2 == 0)
    add("vertical stripes, shifted", xx % 2 == 1)
    add("horizontal stripes", yy % 2 == 0)
    add("horizontal stripes, shifted", yy % 2 == 1)
    # a run of ones / of zeros that continues from the bottom of column 31 into the top of column 32 (where the size has them; else from
    # the bottom of the last but one column into the last, or nothing)
    xa = 31 if W > 32 else W - 2
    ones = z.copy()
    if xa >= 0:
        ones[H - (H + 1) // 2:, xa] = True
        ones[:(H + 1) // 2, xa + 1] = True
    add("ones across the column border", ones)
    add("zeros across the column border", ~ones)
    add("random 0.5", rng.random((H, W)) < 0.5)
    add("random 0.02", rng.random((H, W)) < 0.02)
    return [n for n, _ in out], np.stack([m for _, m in out])


def discs(n, side=1024, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:side, :side].astype(np.float32)
    out = np.zeros((n, side, side), bool)
    for i in range(n):
        cy, cx = rng.uniform(0.1, 0.9, 2) * side
        r = rng.uniform(0.03, 0.3) * side
        out[i] = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return out
