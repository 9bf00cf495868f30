"""saber.analysis.organelle_statistics (saber/analysis/organelle_statistics.py:5-100) on the MI355X: organelle coordinates and size
statistics from a 3-D label volume.

The reference loops over np.unique(mask): per label it builds `(mask == label).astype(int)` over the whole volume, sums it twice and runs
skimage.measure.regionprops on it.  Everything it reports (voxel count, centroid, axis_major_length, axis_minor_length) follows from ten
integer moments per label, which csrc/labelstats.hip gathers for all labels in two reads of the volume (C-ABI: saber_label_statistics).
The sums are integers, so the table is exact and the same bits on every call.

`organelle_table` is the fast path: one small host table over all labels > 0.  `extract_organelle_statistics` keeps the reference's
signature, prints and return value on top of it.  There is no CPU path.

One deliberate deviation: the reference falls back to the equivalent-sphere diameter when skimage's sqrt receives a negative argument
(:52-55).  That happens only for flat labels (every voxel in one plane), where rounding decides the sign of a quantity that is zero in
exact arithmetic, so it is not reproducible.  Here the argument 20 * lambda_min is clamped at 0 (a flat label has axis_minor_length 0)
and there is no fall-back."""
import numpy as np
import torch

from .refine_membranes import MAX_LABEL, _TORCH_OK

MAX_DIM = 65535
MAX_VOXELS = 2 ** 31 - 1


def _check_mask(mask):
    if not isinstance(mask, (np.ndarray, torch.Tensor)):
        raise ValueError(f"mask: expected a numpy array or a torch tensor, got {type(mask).__name__}")
    if mask.ndim != 3:
        raise ValueError(f"mask: expected a 3-D volume, got {mask.ndim}-D")
    is_float = mask.dtype.is_floating_point or mask.dtype.is_complex if isinstance(mask, torch.Tensor) else not (
        np.issubdtype(mask.dtype, np.integer) or mask.dtype == np.bool_)
    if is_float:
        raise ValueError(f"mask: label volumes are integer arrays, got {mask.dtype}")
    shape = tuple(int(s) for s in mask.shape)
    if max(shape) > MAX_DIM or shape[0] * shape[1] * shape[2] >= MAX_VOXELS:
        raise ValueError(f"mask: shape {shape} is over the limits (each axis <= {MAX_DIM}, fewer than 2^31 voxels)")


def _to_device(mask, device):
    """The narrowing of OrganelleMembraneFilter._to_device (bool -> uint8; 64-bit and int8 labels -> int32 after a range check; everything
    else as it is, a contiguous device tensor in place), except that negative values are background here, not an error."""
    t = torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype not in _TORCH_OK:
        if t.numel() and int(t.max()) > MAX_LABEL:
            raise ValueError("organelle labels must lie in [0, 2^22]")
        t = t.clamp(min=-1).to(torch.int32) if t.dtype in (torch.int8, torch.int64) else t.to(torch.int32)
    return t.to(device).contiguous()


def _engine(mask, gpu_id):
    if not torch.cuda.is_available():
        raise RuntimeError("saber_amd.analysis.organelle_statistics needs a ROCm device: there is no CPU fallback")
    from saber_amd.filters._context import handle
    if gpu_id is not None:
        return handle(gpu_id)
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        return handle(mask.device)
    return handle(None)


def organelle_table(mask, gpu_id=None):
    """Every label > 0 of a (Z,H,W) integer volume (numpy or torch; a contiguous device tensor is used in place), ascending, as host arrays:
      label (K,) int64 | count (K,) int64 | centroid (K,3) float64, (z,y,x) | bbox (K,6) int64, zmin ymin xmin zmax ymax xmax, inclusive |
      axis_major_length, axis_minor_length (K,) float64, skimage's definitions | eigenvalues (K,3) float64, descending, of the covariance
      of the voxel coordinates.  Zero and negative values are background."""
    _check_mask(mask)
    eng = _engine(mask, gpu_id)
    vol = _to_device(mask, eng.device)
    if vol.numel() == 0:
        labels, mom, stats = (torch.empty((0,) + s, dtype=d) for s, d in (((), torch.int32), ((16,), torch.int64), ((8,), torch.float64)))
    else:
        with torch.cuda.device(eng.device):
            labels, mom, stats = eng.label_statistics(vol)
    mom, stats = mom.cpu().numpy(), stats.cpu().numpy()
    return {"label": labels.cpu().numpy().astype(np.int64), "count": mom[:, 0].copy(), "centroid": stats[:, 0:3].copy(), "bbox": mom[:, 10:16].copy(),
            "axis_major_length": stats[:, 3].copy(), "axis_minor_length": stats[:, 4].copy(), "eigenvalues": stats[:, 5:8].copy()}


def extract_organelle_statistics(run, mask, organelle_name, session_id, user_id, voxel_size, save_copick=True, save_statistics=True,
                                 xyz_order=True, write_picks=None, gpu_id=None):
    """organelle_statistics.py:5-79.  Returns the CSV rows [run.name, label, volume_nm3, diameter_nm] when save_statistics is set, else [].
    write_picks: see save_coordinates_to_copick."""
    table = organelle_table(mask, gpu_id)
    coordinates = {}
    csv_rows = []
    for i, label in enumerate(table["label"]):
        n = int(table["count"][i])
        if n < 3:                                              # :25
            print(f"Skipping label {label} in {run.name}: too small (< 3 voxels)")
            continue
        centroid = tuple(float(c) for c in table["centroid"][i])
        if xyz_order:
            centroid = centroid[::-1]
        coordinates[str(label)] = centroid
        if save_statistics:
            volume = n * (voxel_size / 10) ** 3                 # Angstrom -> nm^3 (:40)
            axis_x = float(table["axis_minor_length"][i]) * (voxel_size / 10)
            axis_y = float(table["axis_major_length"][i]) * (voxel_size / 10)
            csv_rows.append([run.name, int(label), volume, (axis_x + axis_y) / 2])
    if len(coordinates) > 0:
        if save_copick:
            save_coordinates_to_copick(run, coordinates, organelle_name, session_id, user_id, voxel_size, write_picks=write_picks)
    else:
        print(f"{run.name} didn't have any organelles present!")
    return csv_rows


def save_coordinates_to_copick(run, coordinates, organelle_name, session_id, user_id, voxel_size, write_picks=None):
    """organelle_statistics.py:81-100: one point per label (coordinate * voxel_size) with the identity as orientation.  write_picks(run,
    points, orientations, object_name=, session_id=, user_id=) replaces the reference's run.new_picks(...).from_numpy(points, orientations),
    which stays the default."""
    orientations = np.zeros([len(coordinates), 4, 4])
    orientations[:, :3, :3] = np.identity(3)
    orientations[:, 3, 3] = 1
    points = np.array(list(coordinates.values()))
    points *= voxel_size
    try:
        if write_picks is not None:
            write_picks(run, points, orientations, object_name=organelle_name, session_id=session_id, user_id=user_id)
        else:
            picks = run.new_picks(object_name=organelle_name, session_id=session_id, user_id=user_id)
            picks.from_numpy(points, orientations)
    except Exception as e:
        print(f"Error creating picks for {run.name}: {e}")
