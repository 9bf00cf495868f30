"""CPU: the host side of the slab preparation (saber_amd/utils/volprep.py and the routes into it): argument checks that need no device,
and the numpy routes, which must not notice that the tensor routes exist."""
import ctypes as C

import numpy as np
import pytest
import torch


def test_kernel_entry_points_refuse_bad_arguments_without_a_device(lib):
    buf = (C.c_float * 64)()
    out = (C.c_float * 64)()
    taps = (C.c_float * 65)(*([1.0 / 65] * 65))
    a, b = C.cast(buf, C.c_void_p), C.cast(out, C.c_void_p)
    for ks in (0, 1, 4, 65):
        assert lib.saber_k_correlate1d_zero(a, 0, b, 1, 4, 16, taps, ks, 0, None, None) == -1
        assert b"odd" in lib.saber_k_last_error()
    assert lib.saber_k_correlate1d_zero(a, 7, b, 1, 4, 16, taps, 15, 0, None, None) == -1
    assert lib.saber_k_correlate1d_zero(a, 0, a, 1, 4, 16, taps, 15, 0, None, None) == -1
    assert lib.saber_k_correlate1d_zero(a, 0, b, 1, 0, 16, taps, 15, 0, None, None) == -1
    assert lib.saber_k_correlate1d_zero(a, 0, b, 1, 4, 16, taps, 15, -1, None, None) == -1
    assert lib.saber_k_normalize_minmax(None, 64, a, None) == -1
    assert lib.saber_k_project_mean(a, 4, 4, 4, 2, 2, b, None) == -1
    assert b"non-empty" in lib.saber_k_last_error()
    assert lib.saber_k_project_mean(a, 4, 4, 4, -1, 2, b, None) == -1


def test_kernel_is_the_segmenters_kernel():
    from saber_amd.segmenters import tomo
    from saber_amd.utils import volprep
    assert tomo.make_gaussian_kernel is volprep.make_gaussian_kernel
    w = volprep.make_gaussian_kernel(5)
    assert w.dtype == np.float32 and len(w) == 15 and abs(float(w.sum()) - 1) < 1e-6 and np.array_equal(w, w[::-1])
    assert len(volprep.make_gaussian_kernel(1)) == 3 and len(volprep.make_gaussian_kernel(7)) == 21


def test_tensor_routes_refuse_what_they_cannot_run():
    from saber_amd.filters import gaussian_smoothing
    from saber_amd.utils import preprocessing as preprocess
    from saber_amd.utils import volprep
    x = np.random.default_rng(0).normal(0, 1, (6, 8, 10)).astype(np.float32)
    t = torch.from_numpy(x)
    with pytest.raises(TypeError):
        preprocess.normalize(t)                           # a CPU tensor: the tensor route is the device route
    with pytest.raises(TypeError):
        preprocess.project_tomogram(t, 3, 2)
    with pytest.raises(TypeError):
        volprep.correlate1d_zero(t, volprep.make_gaussian_kernel(5))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        gaussian_smoothing(t, 5)
    assert not volprep.is_device_volume(t) and not volprep.is_device_volume(x)
    # the numpy routes are the reference's expressions
    lo, hi = x.min(), x.max()
    assert np.array_equal(preprocess.normalize(x), (x - lo) / (hi - lo + 1e-8))
    assert np.array_equal(preprocess.project_tomogram(x, 3, 2), np.mean(x[1:5], axis=0))
    assert np.array_equal(preprocess.project_tomogram(x, 3), x[3])
    assert np.array_equal(preprocess.project_tomogram(x), np.mean(x, axis=0))


def test_public_gaussian_smoothing_fails_loudly_without_device():
    if torch.cuda.is_available():
        pytest.skip("has a GPU")
    from saber_amd.filters import gaussian_smoothing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gaussian_smoothing(np.ones((4, 8, 8), np.float32), 5, dim=0)
