"""CPU: the host side of the organelle statistics (saber_amd.analysis.organelle_statistics, the two entry-point bodies) with stub run objects
and injected callables; the device table is replaced by one built from the numpy restatement (tests/organelle_stats_ref.py)."""
import numpy as np
import pytest

import organelle_stats_ref as ref


class StubPicks:
    def __init__(self, log, **kw):
        self.log, self.kw = log, kw

    def from_numpy(self, points, orientations):
        self.log.append((self.kw, np.array(points), np.array(orientations)))


class StubRun:
    def __init__(self, name, seg):
        self.name, self.seg, self.picks = name, seg, []

    def new_picks(self, **kw):
        return StubPicks(self.picks, **kw)


class Obj:
    def __init__(self, name):
        self.name = name


def scene(seed):
    vol = ref.blob_scene((10, 30, 44), seed, n_labels=5, dtype=np.uint16, values=(2, 3, 9, 40, 41))
    vol[0, 0, 0:2] = 77                                       # 2 voxels: skipped
    return vol


def read_seg(run, voxel_size, name, session_id, user_id):
    assert (name, session_id, user_id) == ("mito", "1", "SABER")
    return run.seg


@pytest.fixture
def fake_table(monkeypatch):
    from saber_amd.analysis import organelle_statistics as mod
    calls = []

    def table(mask, gpu_id=None):
        calls.append(mask)
        return ref.table_from_props(ref.label_props(mask))
    monkeypatch.setattr(mod, "organelle_table", table)
    return calls


def csv_bytes(rows):
    out = "run_id,label,volume_nm3,diameter_nm\r\n"
    for name, label, volume, diameter in rows:
        out += f"{name},{label},{volume!r},{diameter!r}\r\n"
    return out.encode()


def test_new_symbols_are_exported(lib):
    import saber_amd.analysis as analysis
    from saber_amd import _lib
    from saber_amd.engine import Engine
    from saber_amd.entry_points import inference_core
    assert "saber_label_statistics" in _lib.SIGNATURES and hasattr(lib, "saber_label_statistics")
    for name in ("organelle_table", "extract_organelle_statistics", "save_coordinates_to_copick"):
        assert name in analysis.__all__ and callable(getattr(analysis, name))
    assert callable(Engine.label_statistics)
    assert callable(inference_core.organelle_statistics_core) and callable(inference_core.process_organelles_core)
    assert "not built" not in analysis.__doc__


def test_organelle_statistics_core_rows_and_picks(fake_table, capsys):
    from saber_amd.entry_points.inference_core import organelle_statistics_core
    vol = scene(1)
    run = StubRun("run_001", vol)
    rows = organelle_statistics_core(run, "mito", "1", "SABER", 7.5, True, True, read_segmentation=read_seg)
    coords, want = ref.expected(vol, "run_001", 7.5)
    assert rows == want and [r[1] for r in rows] == sorted(r[1] for r in rows) and len(rows) >= 3
    assert "Skipping label 77 in run_001: too small (< 3 voxels)" in capsys.readouterr().out
    # the default writer is the reference's run.new_picks(...).from_numpy(points, orientations)
    (kw, points, orientations), = run.picks
    assert kw == dict(object_name="mito", session_id="1", user_id="SABER")
    assert np.array_equal(points, np.array(list(coords.values())) * 7.5)
    assert orientations.shape == (len(coords), 4, 4) and all(np.array_equal(o, np.eye(4)) for o in orientations)
    # an injected writer gets the same arrays
    got = []
    rows2 = organelle_statistics_core(run, "mito", "1", "SABER", 7.5, True, False, read_segmentation=read_seg,
                                      write_picks=lambda r, p, o, **kw: got.append((r, p, o, kw)))
    assert rows2 == [] and len(run.picks) == 1
    assert got[0][0] is run and np.array_equal(got[0][1], points) and got[0][3] == kw
    # save_copick off: no picks
    organelle_statistics_core(run, "mito", "1", "SABER", 7.5, False, True, read_segmentation=read_seg)
    assert len(run.picks) == 1


def test_xyz_order_and_writer_exception(fake_table, capsys):
    from saber_amd.analysis import extract_organelle_statistics
    vol = scene(2)
    run = StubRun("r", vol)
    got = []
    extract_organelle_statistics(run, vol, "mito", "1", "SABER", 10.0, True, False, xyz_order=False,
                                 write_picks=lambda r, p, o, **kw: got.append(p))
    coords, _ = ref.expected(vol, "r", 10.0, xyz_order=False)
    assert np.array_equal(got[0], np.array(list(coords.values())) * 10.0)

    def broken(*a, **kw):
        raise OSError("disk full")
    assert extract_organelle_statistics(run, vol, "mito", "1", "SABER", 10.0, True, True, write_picks=broken) == ref.expected(vol, "r", 10.0)[1]
    assert "Error creating picks for r: disk full" in capsys.readouterr().out


def test_missing_segmentation_and_no_organelles(fake_table, capsys):
    from saber_amd.entry_points.inference_core import organelle_statistics_core
    run = StubRun("run_none", None)
    assert organelle_statistics_core(run, "mito", "1", "SABER", 10.0, True, True, read_segmentation=read_seg) == []
    assert "run_none didn't have any mito segmentations present!" in capsys.readouterr().out
    assert fake_table == []                                  # nothing was computed
    tiny = np.zeros((4, 5, 6), np.uint8)
    tiny[1, 1, 1:3] = 1                                       # only a 2-voxel label
    run = StubRun("run_empty", tiny)
    assert organelle_statistics_core(run, "mito", "1", "SABER", 10.0, True, True, read_segmentation=read_seg) == []
    assert "run_empty didn't have any organelles present!" in capsys.readouterr().out
    assert run.picks == []


def test_process_organelles_core_csv(fake_table, tmp_path, capsys):
    from saber_amd.entry_points.inference_core import process_organelles_core
    runs = [StubRun("run_b", scene(3)), StubRun("run_missing", None), StubRun("run_a", scene(4))]
    out = tmp_path / "stats.csv"
    rows = process_organelles_core(runs, "mito", "1", "SABER", 12.0, True, True, str(out), pickable_objects=[Obj("ribosome"), Obj("mito")],
                                   read_segmentation=read_seg)
    want = ref.expected(runs[0].seg, "run_b", 12.0)[1] + ref.expected(runs[2].seg, "run_a", 12.0)[1]       # run order, then label order
    assert rows == want
    assert out.read_bytes() == csv_bytes(want)
    assert len(runs[0].picks) == 1 and len(runs[2].picks) == 1 and runs[1].picks == []
    text = capsys.readouterr().out
    assert "Statistics saved to" in text and "Coordinate extraction and Statistics calculation complete!" in text
    # no rows at all: the header alone
    out2 = tmp_path / "none.csv"
    assert process_organelles_core([StubRun("x", None)], "mito", "1", "SABER", 12.0, False, True, str(out2), read_segmentation=read_seg) == []
    assert out2.read_bytes() == b"run_id,label,volume_nm3,diameter_nm\r\n"
    # coordinates only: no file
    out3 = tmp_path / "no_file.csv"
    assert process_organelles_core(runs[:1], "mito", "1", "SABER", 12.0, True, False, str(out3), pickable_objects=[Obj("mito")],
                                   read_segmentation=read_seg) == []
    assert not out3.exists() and len(runs[0].picks) == 2


def test_process_organelles_core_errors(fake_table, tmp_path):
    from saber_amd.entry_points.inference_core import process_organelles_core
    runs = [StubRun("run_b", scene(3))]
    with pytest.raises(ValueError, match="At least one of save_copick or save_statistics"):
        process_organelles_core(runs, "mito", "1", "SABER", 12.0, False, False, str(tmp_path / "a.csv"), read_segmentation=read_seg)
    with pytest.raises(ValueError, match="Pickable Object mito not found.*\n.*ribosome, membrane"):
        process_organelles_core(runs, "mito", "1", "SABER", 12.0, True, True, str(tmp_path / "b.csv"),
                                pickable_objects=[Obj("ribosome"), Obj("membrane")], read_segmentation=read_seg)

    class Root:
        pickable_objects = [Obj("mito")]
    assert len(process_organelles_core(runs, "mito", "1", "SABER", 12.0, True, True, str(tmp_path / "c.csv"), pickable_objects=Root(),
                                       read_segmentation=read_seg)) >= 3
    with pytest.raises(ValueError, match="pickable_objects"):
        process_organelles_core(runs, "mito", "1", "SABER", 12.0, True, True, str(tmp_path / "d.csv"), read_segmentation=read_seg)
    assert fake_table and not (tmp_path / "a.csv").exists() and not (tmp_path / "b.csv").exists()


def test_argument_errors_come_first_then_the_loud_no_device_error(monkeypatch):
    import torch
    from saber_amd.analysis import extract_organelle_statistics, organelle_table
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match="3-D"):
        organelle_table(np.ones((8, 8), np.uint16))
    with pytest.raises(ValueError, match="integer"):
        organelle_table(np.ones((4, 8, 8), np.float32))
    with pytest.raises(ValueError, match="integer"):
        organelle_table(torch.ones((4, 8, 8), dtype=torch.float16))
    with pytest.raises(ValueError, match="limits"):
        organelle_table(np.zeros((1, 1, 70000), np.uint8))
    with pytest.raises(ValueError, match="limits"):
        organelle_table(np.broadcast_to(np.uint8(0), (2048, 1024, 1024)))
    with pytest.raises(ValueError, match="numpy array or a torch tensor"):
        organelle_table([[[1]]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        organelle_table(np.ones((4, 8, 8), np.uint16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract_organelle_statistics(StubRun("r", None), np.ones((4, 8, 8), np.int32), "mito", "1", "SABER", 10.0)
