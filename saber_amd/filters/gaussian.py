"""saber.filters.gaussian.gaussian_smoothing (saber/filters/gaussian.py:17-74) and gaussian_smoothing_3d (:76-138) on the MI355X."""
import numpy as np
import torch

from ._context import device_index, handle


def gaussian_smoothing(input_tensor, sigma, dim=-1):
    """1-D Gaussian along `dim` (reference signature): the kernel of make_gaussian_kernel(sigma), zero 'same' padding, fp32
    (saber_k_correlate1d_zero).  numpy in -> float32 numpy out, computed on torch's current device; a CUDA tensor (float32, int16, uint16
    or uint8; anything else is cast to float32 like the reference's .float()) -> a float32 tensor on its device.  The input is not modified."""
    from saber_amd.utils import volprep
    is_tensor = isinstance(input_tensor, torch.Tensor)
    if is_tensor:
        device_index(input_tensor.device)                   # a CPU tensor: "ROCm device only"
        t = input_tensor if input_tensor.dtype in volprep.CORRELATE_DTYPES else input_tensor.float()
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("saber_amd filters run on a ROCm device only (there is no CPU fallback)")
        t = volprep.to_device_volume(np.asarray(input_tensor), torch.device("cuda", device_index(None)))
    if not -t.dim() <= dim < t.dim():
        raise IndexError(f"gaussian_smoothing: dim {dim} out of range for a {t.dim()}-D input")
    out = volprep.correlate1d_zero(t, volprep.make_gaussian_kernel(sigma), dim=dim)
    return out if is_tensor else out.cpu().numpy()


def gaussian_smoothing_3d(volume, sigma, device=None):
    """Separable zero-padded 3-D Gaussian of a binary volume: int(6 sigma + 1) taps (made odd) along x, then y, then z, in fp32.
    volume: 3-D numpy array (bool / 0-1 values, as fast_3d_gaussian_smoothing passes it) or a device tensor; returns the float32
    field as numpy (reference signature) or, for tensor input, as a tensor on the same device."""
    is_tensor = isinstance(volume, torch.Tensor)
    if volume.ndim != 3:
        raise ValueError(f"Expected 3D input, got {volume.ndim}D")
    eng = handle(volume.device if is_tensor else device)
    if is_tensor:
        m = volume
    else:
        v = np.asarray(volume)
        if v.dtype != np.bool_ and not np.isin(v, (0, 1)).all():
            raise ValueError("gaussian_smoothing_3d: the MI355X filter takes a 0/1 mask (what fast_3d_gaussian_smoothing passes)")
        m = torch.from_numpy(np.ascontiguousarray(v.astype(np.uint8))).to(eng.device)
    if m.dtype not in (torch.bool, torch.uint8):
        m = (m != 0)
    with torch.cuda.device(eng.device):
        out = eng.gaussian_smoothing_3d(m.contiguous(), float(sigma))
    return out if is_tensor else out.cpu().numpy()
