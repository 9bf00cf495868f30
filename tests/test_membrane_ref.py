"""CPU: the membrane-refinement fixture (tests/golden/saber_membranes.npz, captured from the reference by
tools/make_golden_membranes.py), the numpy / scipy restatement of the pipeline (tests/membrane_ref.py) and the host side of
saber_amd.analysis.refine_membranes.  Everything is exact equality."""
import json
import os

import numpy as np
import pytest
import torch

import membrane_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "saber_membranes.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["runs"]))


def test_fixture_covers_the_cases(golden):
    g, runs = golden
    assert {r["cfg"]["ball_size"] for r in runs} == {3, 5}
    assert {r["org_dtype"] for r in runs} >= {"uint8", "int32", "int64"}
    assert any(r["cfg"]["edge_trim_z"] == 0 and r["ndim"] == 3 and r["container"] == "torch" for r in runs)
    assert any(r["stacks"] for r in runs)
    assert any(r["cfg"]["keep_surface_membranes"] for r in runs)
    for k, r in enumerate(runs):                               # the +1 shift: outputs only hold input label + 1
        out = set(np.unique(g[f"r{k}_org_out"]).tolist()) - {0}
        assert out <= {int(v) + 1 for v in np.unique(g[f"r{k}_org"]) if v}
    # the pair of runs that differ only in keep_surface_membranes: membranes differ, organelles do not
    a = next(k for k, r in enumerate(runs) if r["cfg"]["ball_size"] == 3 and not r["cfg"]["keep_surface_membranes"] and r["cfg"]["edge_trim_z"] == 5)
    b = next(k for k, r in enumerate(runs) if r["cfg"] == dict(runs[a]["cfg"], keep_surface_membranes=True))
    assert (g[f"r{a}_mem_out"] != g[f"r{b}_mem_out"]).any() and (g[f"r{a}_org_out"] == g[f"r{b}_org_out"]).all()


def test_restatement_reproduces_every_fixture(golden):
    g, runs = golden
    for k, r in enumerate(runs):
        org, mem = g[f"r{k}_org"], g[f"r{k}_mem"]
        pairs, _ = membrane_ref.refine(org.astype(r["org_dtype"]), mem, **r["cfg"])
        o3, m3 = membrane_ref.flatten(pairs, org.shape)
        assert len(pairs) == r["n_pairs"], (k, r)
        assert int((o3 != g[f"r{k}_org_out"]).sum()) == 0 and int((m3 != g[f"r{k}_mem_out"]).sum()) == 0, (k, r)
        if r["stacks"]:
            o4, m4 = membrane_ref.stacks(pairs, org.shape)
            assert np.array_equal(o4, g[f"r{k}_org_stack"]) and np.array_equal(m4, g[f"r{k}_mem_stack"]), (k, r)


def test_roi_threshold_is_float32():
    thr = membrane_ref.roi_thresholds((64, 160, 200), 0.15)
    assert thr.dtype == np.float32 and thr[1] == np.float32(24.0) and thr[0] > np.float32(9.6) - 1e-6 and thr[2] > 30.0
    from saber_amd.analysis.refine_membranes import OrganelleMembraneFilter
    p = OrganelleMembraneFilter()._params((64, 160, 200))
    assert [np.float32(v) for v in p.min_roi_size] == [np.float32(v) for v in thr]


def test_module_imports_and_defaults_match_the_reference(golden):
    g, _ = golden
    from saber_amd.analysis import FilteringConfig, OrganelleMembraneFilter       # noqa: F401
    import dataclasses
    mine = dataclasses.asdict(FilteringConfig())
    assert mine == json.loads(str(g["defaults"]))


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("has a GPU")
    from saber_amd.analysis import OrganelleMembraneFilter
    f = OrganelleMembraneFilter()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f.run(np.ones((12, 16, 16), np.uint8), np.ones((12, 16, 16), np.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f.run_labels(np.ones((12, 16, 16), np.uint8), np.ones((12, 16, 16), np.uint8))
    with pytest.raises(ValueError):                            # the argument checks come first
        f.run(np.ones((16, 16), np.uint8), np.ones((16, 16), np.uint8))
    with pytest.raises(ValueError):
        f.run(np.ones((12, 16, 16), np.uint8), np.ones((12, 16, 17), np.uint8))
    with pytest.raises(ValueError):
        f.run(np.ones((12, 16, 16), np.float32), np.ones((12, 16, 16), np.uint8))


def test_convert_to_3d_labels_on_the_stored_stacks(golden):
    g, runs = golden
    from saber_amd.analysis import OrganelleMembraneFilter
    f = OrganelleMembraneFilter()
    seen = 0
    for k, r in enumerate(runs):
        if not r["stacks"]:
            continue
        seen += 1
        for kind in ("org", "mem"):
            stack = g[f"r{k}_{kind}_stack"]
            flat = f.convert_to_3d_labels(stack)
            assert isinstance(flat, np.ndarray) and flat.dtype == stack.dtype and np.array_equal(flat, g[f"r{k}_{kind}_out"])
            flat_t = f.convert_to_3d_labels(torch.from_numpy(stack))
            assert isinstance(flat_t, torch.Tensor) and np.array_equal(flat_t.numpy(), g[f"r{k}_{kind}_out"])
    assert seen >= 2
    # later planes overwrite earlier ones
    st = np.zeros((2, 1, 2, 2), np.uint8)
    st[0, 0, 0, :] = 2
    st[1, 0, :, 0] = 3
    assert f.convert_to_3d_labels(st).tolist() == [[[3, 2], [3, 0]]]
