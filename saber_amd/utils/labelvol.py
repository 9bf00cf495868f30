"""Propagated label volumes on the device (csrc/labelvol.hip): the stages between the video tracking loop and the 3-D stitch - one paint
launch per frame, the presence filter as a per-frame table look-up, and the merges of the segmenters that seed several slices - on
device tensors.  SAM2Adapter.segment_volume(device_volume=True) and the segmenters with device_volumes = True come this way; numpy
volumes never do.  Label volumes are int16 / uint16 tensors holding uint16 values (what Engine.separate_masks accepts)."""
import ctypes as C

import numpy as np
import torch

from saber_amd import _lib

LABEL_DTYPES = (torch.int16, torch.uint16)


def require_device(device, what: str) -> torch.device:
    """`device` as a torch.device; without a ROCm device this is the package's "no CPU fallback" error."""
    d = torch.device(device)
    if d.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"{what} needs a ROCm device, got '{d}' (torch.cuda.is_available() is {torch.cuda.is_available()}); "
                           "there is no CPU fallback (leave the device route off for the host route)")
    return d


def presence_keep_table(bounds, min_presence_score: float) -> np.ndarray:
    """The presence filter of SAM2Adapter.segment_volume as a look-up table.  bounds: (Z, n) presence scores of object id j + 1 on
    frame z (fit_organelle_boundaries).  Returns (Z, n + 1) uint16: table[z][id] = id where the object stays on that frame, 0 where
    bounds[z][id - 1] < min_presence_score (a score equal to the threshold stays, as in the reference); column 0 is background, 0 -> 0."""
    b = np.asarray(bounds, dtype=np.float64)
    if b.ndim != 2:
        raise ValueError(f"presence_keep_table: expected (Z, n) scores, got {b.shape}")
    Z, n = b.shape
    if n + 1 > 65536:
        raise ValueError("presence_keep_table: object ids do not fit uint16")
    table = np.zeros((Z, n + 1), dtype=np.uint16)
    ids = np.arange(1, n + 1, dtype=np.uint16)
    table[:, 1:] = np.where(b < min_presence_score, np.uint16(0), ids[None, :])
    return table


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _check(lib, status: int) -> None:
    if status != 0:
        raise RuntimeError(lib.saber_k_last_error().decode())


def _need(t, what: str, dtypes, like: torch.Tensor = None) -> None:
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError(f"{what}: expected a CUDA tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"{what}: unsupported element type {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous tensor")
    if like is not None and (t.device != like.device or t.numel() != like.numel()):
        raise ValueError(f"{what}: tensors must lie on one device and have the same number of elements")


def paint_nearest_stack(logits: torch.Tensor, labels, plane: torch.Tensor, thr: float = 0.0, any_flag: torch.Tensor = None) -> None:
    """plane (H,W) <- labels[i] wherever logits[i] > thr at the nearest source pixel, the last such i winning: all objects of a frame in
    one launch.  logits: (n,Hv,Wv) or (n,1,Hv,Wv) float32; labels: n ints; any_flag: optional device int32, OR-ed with 1 on a write."""
    _need(logits, "paint_nearest_stack", (torch.float32,))
    _need(plane, "paint_nearest_stack", LABEL_DTYPES)
    if plane.dim() != 2 or logits.dim() < 3 or plane.device != logits.device:
        raise ValueError("paint_nearest_stack: expected (n,Hv,Wv) logits and an (H,W) plane on one device")
    n = int(logits.shape[0])
    Hv, Wv = (int(v) for v in logits.shape[-2:])
    if logits.numel() != n * Hv * Wv or len(labels) != n:
        raise ValueError("paint_nearest_stack: one (Hv,Wv) plane and one label per object are needed")
    if n == 0:
        return
    lab = (C.c_int * n)(*[int(v) for v in labels])
    lib = _lib.load()
    with torch.cuda.device(plane.device):
        _check(lib, lib.saber_k_paint_nearest_stack(C.c_void_p(logits.data_ptr()), n, Hv, Wv, lab, float(thr), C.c_void_p(plane.data_ptr()),
                                                    int(plane.shape[0]), int(plane.shape[1]),
                                                    None if any_flag is None else C.c_void_p(any_flag.data_ptr()), _stream(plane)))


def relabel_frames_(vol: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """vol[z] <- lut[z][vol[z]] in place for values below lut.shape[1] (larger values stay); vol (Z,...) labels, lut (Z,L); returns vol"""
    _need(vol, "relabel_frames_", LABEL_DTYPES)
    _need(lut, "relabel_frames_", LABEL_DTYPES)
    if vol.dim() < 2 or lut.dim() != 2 or lut.shape[0] != vol.shape[0] or lut.device != vol.device:
        raise ValueError("relabel_frames_: expected a (Z,...) volume and a (Z,L) table on its device")
    if vol.numel() == 0:
        return vol
    Z = int(vol.shape[0])
    lib = _lib.load()
    with torch.cuda.device(vol.device):
        _check(lib, lib.saber_k_relabel_frames(C.c_void_p(vol.data_ptr()), Z, vol.numel() // Z, C.c_void_p(lut.data_ptr()), int(lut.shape[1]), _stream(vol)))
    return vol


def merge_max_u16_(acc: torch.Tensor, src: torch.Tensor, binarize: bool = False) -> torch.Tensor:
    """acc <- max(acc, src > 0 if binarize else src) in place as uint16 values; returns acc"""
    _need(acc, "merge_max_u16_", LABEL_DTYPES)
    _need(src, "merge_max_u16_", LABEL_DTYPES, like=acc)
    lib = _lib.load()
    with torch.cuda.device(acc.device):
        _check(lib, lib.saber_k_merge_max_u16(C.c_void_p(acc.data_ptr()), C.c_void_p(src.data_ptr()), acc.numel(), int(bool(binarize)), _stream(acc)))
    return acc


def merge_class_conf_(final: torch.Tensor, best: torch.Tensor, src: torch.Tensor, cls: torch.Tensor, conf: torch.Tensor) -> None:
    """Where v = src > 0 indexes the tables and conf[v] > best (strictly): final <- cls[v], best <- conf[v], both in place.  cls (L)
    labels and conf (L) float32 on the device, indexed by object id; entry 0 is never applied."""
    _need(final, "merge_class_conf_", LABEL_DTYPES)
    _need(best, "merge_class_conf_", (torch.float32,), like=final)
    _need(src, "merge_class_conf_", LABEL_DTYPES, like=final)
    _need(cls, "merge_class_conf_", LABEL_DTYPES)
    _need(conf, "merge_class_conf_", (torch.float32,), like=cls)
    if cls.device != final.device or cls.numel() == 0:
        raise ValueError("merge_class_conf_: the tables must lie on the volume's device and hold at least entry 0")
    lib = _lib.load()
    with torch.cuda.device(final.device):
        _check(lib, lib.saber_k_merge_class_conf(C.c_void_p(final.data_ptr()), C.c_void_p(best.data_ptr()), C.c_void_p(src.data_ptr()),
                                                 C.c_void_p(cls.data_ptr()), C.c_void_p(conf.data_ptr()), int(cls.numel()), final.numel(), _stream(final)))
