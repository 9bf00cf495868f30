"""saber.analysis.refine_membranes.OrganelleMembraneFilter (saber/analysis/refine_membranes.py:54-590) on the MI355X.

The reference trims and cleans the membrane segmentation, then, per organelle label: cuts a padded ROI, dilates membrane and organelle,
keeps the membrane near the organelle, opens `organelle OR membrane` with a ball and uses the largest component of the result to
constrain both.  It does so with dense fp32 conv3d morphology, scipy.ndimage.label on the host and a clone of the volume per organelle.
Here the whole pipeline is csrc/morph3d.hip (bit-packed ball morphology, 6-connected union-find) behind one C-ABI call with three host
synchronisations; the results are bit-identical.

Two things a caller must know (both are the reference's behaviour, reproduced):
  * output labels are shifted by one: organelle v comes out as v + 1, in the organelle and in the membrane output;
  * `ball_size` is a radius.

`run` returns what the reference returns (4-D stacks on the host).  `run_labels` is the fast path: the two flattened 3-D label maps as
device tensors, which is what the entry point saves.  There is no CPU path."""
from dataclasses import dataclass

import numpy as np
import torch

from saber_amd import _lib

_TORCH_OK = (torch.uint8, torch.int16, torch.uint16, torch.int32, torch.uint32)
MAX_LABEL = 2 ** 22


@dataclass
class FilteringConfig:
    """Same fields and defaults as the reference (refine_membranes.py:54-63)."""
    ball_size: int = 3
    min_membrane_area: int = 10000
    edge_trim_z: int = 5
    edge_trim_xy: int = 3
    min_roi_relative_size: float = 0.15
    batch_size: int = 8
    keep_surface_membranes: bool = False


class OrganelleMembraneFilter:
    def __init__(self, config: FilteringConfig = None, gpu_id: int = None):
        self.config = config or FilteringConfig()
        self.gpu_id = gpu_id

    # ------------------------------------------------------------------ argument handling
    def _check_config(self):
        c = self.config
        if not 1 <= int(c.ball_size) <= 16:
            raise ValueError(f"ball_size is a radius and must lie in 1..16, got {c.ball_size}")
        if int(c.edge_trim_z) < 0 or int(c.edge_trim_xy) < 0:
            raise ValueError("edge trims must not be negative")
        if int(c.batch_size) < 1:
            raise ValueError(f"batch_size must be positive, got {c.batch_size}")

    @staticmethod
    def _check_volumes(organelle_seg, membrane_seg):
        for name, a in (("organelle_seg", organelle_seg), ("membrane_seg", membrane_seg)):
            if not isinstance(a, (np.ndarray, torch.Tensor)):
                raise ValueError(f"{name}: expected a numpy array or a torch tensor, got {type(a).__name__}")
            if a.ndim != 3:
                raise ValueError(f"{name}: expected a 3-D volume, got {a.ndim}-D")
        if tuple(organelle_seg.shape) != tuple(membrane_seg.shape):
            raise ValueError(f"organelle and membrane volumes differ in shape: {tuple(organelle_seg.shape)} vs {tuple(membrane_seg.shape)}")
        is_float = organelle_seg.dtype.is_floating_point if isinstance(organelle_seg, torch.Tensor) else not (
            np.issubdtype(organelle_seg.dtype, np.integer) or organelle_seg.dtype == np.bool_)
        if is_float:
            raise ValueError(f"organelle_seg: label volumes are integer arrays, got {organelle_seg.dtype}")

    def _engine(self, organelle_seg):
        if not torch.cuda.is_available():
            raise RuntimeError("saber_amd.analysis.refine_membranes needs a ROCm device: there is no CPU fallback")
        from saber_amd.filters._context import handle
        if self.gpu_id is not None:
            return handle(self.gpu_id)
        if isinstance(organelle_seg, torch.Tensor) and organelle_seg.is_cuda:
            return handle(organelle_seg.device)
        return handle(None)

    @staticmethod
    def _to_device(a, device, labels: bool):
        """Narrow / view the way saber_amd.filters does: bool -> uint8, 64-bit and int8 labels -> int32, everything else as it is."""
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        if not labels:
            t = t.to(device)
            return (t if t.dtype in (torch.bool, torch.uint8) else (t != 0)).contiguous()
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        if t.dtype not in _TORCH_OK:                          # int64, int8, uint64: through int32 after a range check
            if t.numel() and (int(t.min()) < 0 or int(t.max()) > MAX_LABEL):
                raise ValueError("organelle labels must lie in [0, 2^22]")
            t = t.to(torch.int32)
        elif t.dtype in (torch.int16, torch.int32) and t.numel() and int(t.min()) < 0:
            raise ValueError("organelle labels must not be negative")
        return t.to(device).contiguous()

    def _params(self, shape) -> "_lib.RefineParams":
        c = self.config
        # the reference's own arithmetic (:262-263): python float * int64 tensor -> float32
        min_sizes = c.min_roi_relative_size * torch.tensor(tuple(shape))
        p = _lib.RefineParams(int(c.ball_size), int(c.min_membrane_area), int(c.edge_trim_z), int(c.edge_trim_xy), int(bool(c.keep_surface_membranes)))
        for i in range(3):
            p.min_roi_size[i] = float(min_sizes[i])
        return p

    def _refine(self, organelle_seg, membrane_seg):
        self._check_config()
        self._check_volumes(organelle_seg, membrane_seg)
        eng = self._engine(organelle_seg)
        org = self._to_device(organelle_seg, eng.device, labels=True)
        mem = self._to_device(membrane_seg, eng.device, labels=False)
        # (largest label + 1) * 2 must fit the caller's dtype: the reference wraps silently there.  The C-ABI checks the unsigned device
        # type (uint8, uint16) and labels <= 2^22 always fit 32 bits; only the signed narrow types need a look of their own.
        if str(organelle_seg.dtype).replace("torch.", "") in ("int8", "int16") and org.numel():
            top = (int(org.max()) + 1) * 2
            if top > 2 and top > (127 if "int8" in str(organelle_seg.dtype) else 32767):
                raise ValueError(f"(largest label + 1) * 2 = {top} does not fit {organelle_seg.dtype}")
        with torch.cuda.device(eng.device):
            org_labels, mem_labels, n_pairs = eng.refine_membranes(org, mem, self._params(org.shape))
        return eng, org_labels, mem_labels, n_pairs

    # ------------------------------------------------------------------ public
    def run_labels(self, organelle_seg, membrane_seg):
        """The two flattened label maps ((Z,H,W) device tensors of the narrowed organelle dtype): convert_to_3d_labels of what `run`
        returns, without ever building the 4-D stacks."""
        _, org_labels, mem_labels, _ = self._refine(organelle_seg, membrane_seg)
        return org_labels, mem_labels

    def run(self, organelle_seg, membrane_seg, batch_processing: bool = False):
        """{'organelles': (K,Z,H,W), 'membranes': (K,Z,H,W)}: one plane per surviving organelle, ascending label, in the organelle
        input's dtype, on the host; numpy for numpy input.  When nothing survives both entries are 3-D zero torch tensors (the
        reference's quirk, :482-489 and :525-532)."""
        is_numpy_org, is_numpy_mem = isinstance(organelle_seg, np.ndarray), isinstance(membrane_seg, np.ndarray)
        eng, org_labels, _, n_pairs = self._refine(organelle_seg, membrane_seg)
        out_dtype = torch.from_numpy(np.empty(0, organelle_seg.dtype)).dtype if is_numpy_org else organelle_seg.dtype
        shape = tuple(org_labels.shape)
        if n_pairs == 0:
            empty = torch.zeros(shape, dtype=out_dtype)
            return {"organelles": empty, "membranes": empty}
        org4 = torch.empty((n_pairs,) + shape, dtype=out_dtype)
        mem4 = torch.empty((n_pairs,) + shape, dtype=out_dtype)
        step = int(self.config.batch_size)
        with torch.cuda.device(eng.device):
            for first in range(0, n_pairs, step):                # batch_size planes at a time: the device never holds K volumes
                count = min(step, n_pairs - first)
                o, m = eng.refine_membranes_instances(first, count, shape, org_labels.dtype)
                org4[first:first + count] = o.cpu().view(_signed(o.dtype)).to(out_dtype)
                mem4[first:first + count] = m.cpu().view(_signed(m.dtype)).to(out_dtype)
        return {"organelles": org4.numpy() if is_numpy_org else org4, "membranes": mem4.numpy() if is_numpy_mem else mem4}

    def convert_to_3d_labels(self, masks_4d):
        """4-D instance stack -> 3-D label map, later planes overwriting earlier ones (:549-573).  Host code."""
        if isinstance(masks_4d, np.ndarray):
            out = np.zeros(masks_4d.shape[1:], dtype=masks_4d.dtype)
        else:
            out = torch.zeros(masks_4d.shape[1:], dtype=masks_4d.dtype, device=masks_4d.device)
        for mask in masks_4d:
            out[mask > 0] = mask[mask > 0]
        return out


def _signed(dtype):
    """uint16 / uint32 device results are re-read as the signed type of the same width before the host conversion (values fit)."""
    return {torch.uint16: torch.int16, torch.uint32: torch.int32}.get(dtype, dtype)
