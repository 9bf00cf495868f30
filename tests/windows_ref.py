"""Host restatement of csrc/windows.hip from bool arrays (numpy only): window-sized masks packed in the generator's layout, pasted into
full frames as saber2D.rasterize_masks pastes them, and stacked as filters.masks.masks_to_array stacks them.  Bit b of word k of a row is
pixel 32k + b."""
import numpy as np

TABLE_DTYPE = np.dtype([("src_word", "<i8"), ("y0", "<i4"), ("x0", "<i4"), ("h", "<i4"), ("w", "<i4")])     # saber_window_mask, 24 bytes


def pack_rows(masks: np.ndarray, padding: bool = False) -> np.ndarray:
    """(..., h, w) bool -> (..., h, ceil(w/32)) uint32; padding=True sets the bits at x >= w of every row's last word"""
    masks = np.asarray(masks, dtype=bool)
    w = masks.shape[-1]
    w32 = (w + 31) // 32
    full = np.full(masks.shape[:-1] + (w32 * 32,), bool(padding))
    full[..., :w] = masks
    packed = np.packbits(full, axis=-1, bitorder="little")          # byte j of a row = pixels 8j .. 8j+7, pixel 8j in bit 0
    return np.ascontiguousarray(packed).view("<u4").astype(np.uint32)


def unpack_rows(words: np.ndarray, w: int) -> np.ndarray:
    """(..., h, w32) uint32 -> (..., h, w) bool"""
    words = np.ascontiguousarray(words, dtype="<u4")
    bits = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")
    return bits[..., :w].astype(bool)


def pack_window(mask: np.ndarray, padding: bool = False) -> np.ndarray:
    """one (h, w) bool window mask -> its h * ceil(w/32) words, row-major"""
    return pack_rows(mask, padding).reshape(-1)


def build_source(masks, offsets, padding: bool = False):
    """window masks (list of (h, w) bool) at offsets (list of (y0, x0)) -> (src uint32 1-D, table as a TABLE_DTYPE array), rows one after another"""
    words, table, at = [], np.zeros(len(masks), dtype=TABLE_DTYPE), 0
    for i, (m, (y0, x0)) in enumerate(zip(masks, offsets)):
        p = pack_window(m, padding)
        table[i] = (at, y0, x0, m.shape[0], m.shape[1])
        words.append(p)
        at += p.size
    src = np.concatenate(words) if words else np.zeros(0, dtype=np.uint32)
    return src.astype(np.uint32), table


def window_masks_of(src: np.ndarray, table) -> list:
    """the inverse of build_source: the bool window masks a (src, table) pair holds (padding bits ignored)"""
    out = []
    for r in table:
        s, y0, x0, h, w = (int(v) for v in r)
        w32 = (w + 31) // 32
        out.append(unpack_rows(np.asarray(src[s:s + h * w32], dtype=np.uint32).reshape(h, w32), w))
    return out


def paste(masks, offsets, H: int, W: int) -> np.ndarray:
    """(n, H, W) bool: every window mask in its own full frame, zero elsewhere"""
    full = np.zeros((len(masks), H, W), dtype=bool)
    for i, (m, (y0, x0)) in enumerate(zip(masks, offsets)):
        full[i, y0:y0 + m.shape[0], x0:x0 + m.shape[1]] = m
    return full


def place(masks, offsets, H: int, W: int) -> np.ndarray:
    """(n, H, ceil(W/32)) uint32: the full-frame arrays packed with clean padding"""
    return pack_rows(paste(masks, offsets, H, W), padding=False)


def label_stack(masks, offsets, H: int, W: int, first: int = 0, count=None, total=None) -> np.ndarray:
    """planes first .. first + count - 1 of masks_to_array on the pasted arrays: plane j holds j + 1, in the narrowest unsigned type that holds
    `total` masks (default: all of them)"""
    n = len(masks)
    total = n if total is None else total
    count = n - first if count is None else count
    dtype = np.uint8 if total < 256 else (np.uint16 if total < 65536 else np.uint32)
    full = paste(masks[first:first + count], offsets[first:first + count], H, W)
    return full.astype(dtype) * np.arange(first + 1, first + count + 1, dtype=dtype)[:, None, None]
