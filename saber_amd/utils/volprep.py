"""Slab preparation on the device (csrc/volprep.hip): the three whole-volume steps in front of tomoSegmenter's per-slice work -
1-D Gaussian along one axis with fused min / max, min-max normalisation in place, slab projection - on device tensors.  The public
functions that route tensors here are saber_amd.filters.gaussian.gaussian_smoothing and saber_amd.utils.preprocessing.normalize /
project_tomogram; numpy input never comes this way."""
import ctypes as C
import math

import numpy as np
import torch

from saber_amd import _lib

# the MRC modes saber_k_correlate1d_zero widens in the kernel
CORRELATE_DTYPES = {torch.float32: 0, torch.int16: 1, torch.uint16: 2, torch.uint8: 3}


def make_gaussian_kernel(sigma: float) -> np.ndarray:
    """Kernel of the reference (filters/gaussian.py:7-15): odd size max(round(3 sigma), 3), taps on linspace(-ks/2, ks/2, ks)."""
    ks = max(round(sigma * 3), 3)
    ks += 1 - ks % 2
    ts = np.linspace(-ks / 2, ks / 2, ks, dtype=np.float32)
    g = np.exp(-(ts / np.float32(sigma)) ** 2 / 2).astype(np.float32)
    return g / g.sum()


def is_device_volume(vol) -> bool:
    """a CUDA tensor of one of the element types the smoothing kernel reads"""
    return isinstance(vol, torch.Tensor) and vol.is_cuda and vol.dtype in CORRELATE_DTYPES


def to_device_volume(vol, device) -> torch.Tensor:
    """one upload of a host tomogram in its own element type where the smoothing kernel reads it (the MRC modes), else as float32 - the
    type the host route casts to; a tensor is moved to `device`"""
    if isinstance(vol, torch.Tensor):
        return vol.to(device)
    a = np.ascontiguousarray(vol)
    if a.dtype == np.uint16:                              # torch.from_numpy has no uint16 on every build
        return torch.from_numpy(a.view(np.int16)).to(device).view(torch.uint16)
    if a.dtype not in (np.float32, np.int16, np.uint8):
        a = a.astype(np.float32)
    return torch.from_numpy(a).to(device)


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _check(lib, status: int) -> None:
    if status != 0:
        raise RuntimeError(lib.saber_k_last_error().decode())


def _need_cuda(t, what: str, dtypes) -> None:
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError(f"{what}: expected a CUDA tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"{what}: unsupported element type {t.dtype}")


def correlate1d_zero(t: torch.Tensor, taps, dim: int = 0, minmax: bool = False, chunk_len: int = 0):
    """scipy.ndimage.correlate1d(t, taps, axis=dim, mode="constant") in fp32 on the device; `t` is not modified.  Returns the float32
    tensor, with minmax=True also a 2-element device tensor (min, max of the result) computed in the same pass."""
    _need_cuda(t, "correlate1d_zero", CORRELATE_DTYPES)
    if t.dim() < 1 or t.numel() == 0:
        raise ValueError("correlate1d_zero: empty input")
    dim = dim % t.dim()
    w = np.ascontiguousarray(taps, dtype=np.float32).ravel()
    t = t.contiguous()
    shape = tuple(t.shape)
    outer, length, inner = math.prod(shape[:dim]), shape[dim], math.prod(shape[dim + 1:])
    lib = _lib.load()
    with torch.cuda.device(t.device):
        out = torch.empty(shape, dtype=torch.float32, device=t.device)
        mm = torch.empty(2, dtype=torch.float32, device=t.device) if minmax else None
        _check(lib, lib.saber_k_correlate1d_zero(C.c_void_p(t.data_ptr()), CORRELATE_DTYPES[t.dtype], C.c_void_p(out.data_ptr()), outer, length, inner,
                                                 w.ctypes.data_as(C.POINTER(C.c_float)), int(w.size), int(chunk_len),
                                                 C.c_void_p(mm.data_ptr()) if minmax else None, _stream(t)))
    return (out, mm) if minmax else out


def normalize_minmax_(t: torch.Tensor, minmax: torch.Tensor) -> torch.Tensor:
    """t <- (t - lo) / (hi - lo + 1e-8) in place with (lo, hi) = the two device floats of `minmax`; returns t"""
    _need_cuda(t, "normalize_minmax_", (torch.float32,))
    _need_cuda(minmax, "normalize_minmax_", (torch.float32,))
    if not t.is_contiguous() or minmax.numel() != 2 or not minmax.is_contiguous() or minmax.device != t.device:
        raise ValueError("normalize_minmax_: a contiguous tensor and two contiguous floats on its device are needed")
    if t.numel() == 0:
        return t
    lib = _lib.load()
    with torch.cuda.device(t.device):
        _check(lib, lib.saber_k_normalize_minmax(C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(minmax.data_ptr()), _stream(t)))
    return t


def project_mean(vol: torch.Tensor, z0: int, z1: int) -> torch.Tensor:
    """mean of the planes z0 .. z1-1 of a (Z,H,W) float32 device volume: numpy's ascending fp32 sum and one division"""
    _need_cuda(vol, "project_mean", (torch.float32,))
    if vol.dim() != 3:
        raise ValueError(f"project_mean: expected (Z,H,W), got {tuple(vol.shape)}")
    vol = vol.contiguous()
    Z, H, W = vol.shape
    lib = _lib.load()
    with torch.cuda.device(vol.device):
        out = torch.empty((H, W), dtype=torch.float32, device=vol.device)
        _check(lib, lib.saber_k_project_mean(C.c_void_p(vol.data_ptr()), Z, H, W, int(z0), int(z1), C.c_void_p(out.data_ptr()), _stream(vol)))
    return out
