"""CPU: fixture archives in parts (saber_amd.utils.npz_parts) read back bit for bit, and every fixture file stays below 1 MiB."""
import os

import numpy as np

from saber_amd.utils import npz_parts

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def test_round_trip_in_parts(tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"big": rng.standard_normal((700, 1000)).astype(np.float32), "bits": rng.integers(0, 2, (64, 512), dtype=np.uint8),
              "n": np.array(3), "name": np.array("fixture")}
    path = str(tmp_path / "a.npz")
    files = npz_parts.save(path, arrays)
    assert len(files) > 1 and not os.path.exists(path) and npz_parts.exists(path)
    assert all(os.path.getsize(f) < npz_parts.LIMIT for f in files)
    back = npz_parts.load(path)
    assert list(back) == list(arrays)
    for k, a in arrays.items():
        assert back[k].dtype == a.dtype and back[k].shape == a.shape and back[k].tobytes() == a.tobytes(), k
    small = str(tmp_path / "b.npz")
    assert npz_parts.save(small, {"n": np.arange(5)}) == [small]
    assert np.array_equal(npz_parts.load(small)["n"], np.arange(5))


def test_golden_files_below_the_limit():
    names = os.listdir(GOLDEN)
    assert names
    for n in names:
        assert os.path.getsize(os.path.join(GOLDEN, n)) < npz_parts.LIMIT, n
    assert npz_parts.exists(os.path.join(GOLDEN, "decoder_fit_large_seed0.npz"))
