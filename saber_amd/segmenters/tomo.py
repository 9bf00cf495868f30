"""tomoSegmenter (reference: saber/segmenters/tomo.py:14-139).  segment_slab's 2-D path (z-smoothing -> normalise ->
slab projection -> segment_image) feeds segment_vol, which continues into SAM2 video propagation on the engine
(SAM2Adapter.segment_volume, saber_amd/adapters/sam2/video.py).  The z Gaussian (filters/gaussian.py:17-74, sigma 5, conv1d) is
glue outside the per-slice loop.  For a numpy volume it is host glue, evaluated with scipy's separable filter of the same kernel; for a
CUDA tensor (float32, int16, uint16, uint8) the whole preparation runs on the device (saber_amd/utils/volprep.py, csrc/volprep.hip):
smoothing with fused min / max, normalisation in place, projection - and the volume goes to the video path where it lies."""
from typing import Optional

import numpy as np
import torch

from saber_amd.adapters.base import AdapterConfig
from saber_amd.adapters.sam2.amg import cfgAMG
from saber_amd.segmenters.base import saber3D
from saber_amd.utils import preprocessing as preprocess
from saber_amd.utils import volprep
from saber_amd.utils.volprep import make_gaussian_kernel


def gaussian_smoothing_z(vol: np.ndarray, sigma: float, dim: int = 0) -> np.ndarray:
    """1-D Gaussian along `dim`: conv1d with zero 'same' padding of the reference kernel (filters/gaussian.py:17-74)."""
    from scipy.ndimage import correlate1d
    return correlate1d(np.asarray(vol, dtype=np.float32), make_gaussian_kernel(sigma), axis=dim, mode="constant", cval=0.0)


class tomoSegmenter(saber3D):
    def __init__(self, deviceID: int = 0, cfg: Optional[AdapterConfig] = None, amg_cfg: Optional[cfgAMG] = None, min_mask_area: int = 50):
        super().__init__(deviceID=deviceID, cfg=cfg, amg_cfg=amg_cfg, min_mask_area=min_mask_area)
        self.filter_threshold = 0.5
        self._prepared = None               # (the volume, prepare_volume of it) while one call segments several slabs of it

    @torch.inference_mode()
    def prepare_volume(self, vol):
        """The part of segment_slab that does not depend on the slab: z-Gaussian (sigma 5) and normalisation of the whole volume, on the
        host for a numpy volume, on the device for a CUDA tensor.  `vol` itself is only read."""
        if isinstance(vol, torch.Tensor):
            if not volprep.is_device_volume(vol) or vol.dim() != 3:
                raise TypeError("segment_slab: a tensor volume must be a (Z,H,W) CUDA tensor of float32, int16, uint16 or uint8")
            # the smoothed copy is this segmenter's own, so it is normalised in place
            smoothed, minmax = volprep.correlate1d_zero(vol, make_gaussian_kernel(5), dim=0, minmax=True)
            return preprocess.normalize_(smoothed, minmax)
        return preprocess.normalize(gaussian_smoothing_z(vol, 5, dim=0))

    @torch.inference_mode()
    def segment_slab(self, vol, slab_thickness: int = 10, zSlice: Optional[int] = None, display: bool = True,
                     text: Optional[str] = None, target_class: Optional[int] = 1):
        if self._prepared is not None and self._prepared[0] is vol:
            self.vol = self._prepared[1]
        else:
            self.vol = self.prepare_volume(vol)
        if zSlice is None:
            zSlice = int(self.vol.shape[0] // 2)
        self.image0 = preprocess.project_tomogram(self.vol, zSlice, slab_thickness)
        self.segment_image(self.image0, display=display, text_prompt=text, target_class=target_class)
        return self.masks

    def segment(self, vol, thickness: int = 10, zSlice: int = None, text: Optional[str] = None, target_class: Optional[int] = 1,
                save_run: str = None, display: bool = False):
        return self.segment_vol(vol, thickness, zSlice, text, target_class, save_run, display)

    @torch.inference_mode()
    def segment_vol(self, vol, thickness: int, zSlice: int = None, text: Optional[str] = None, target_class: Optional[int] = 1,
                    save_run: str = None, display: bool = False):
        self.is_tomogram_mode = True
        self.segment_slab(vol, thickness, zSlice, display=False, text=text, target_class=target_class)
        if len(self.masks) == 0:
            return None
        # the reference loads the volume once per segmenter (`_vol_loaded` is never reset, tomo.py:117-119), so a pooled segmenter
        # propagates its FIRST tomogram's frames for every later one (known reference bug): here every call loads its own
        self.video_predictor.set_volume(self.vol)
        self._vol_loaded = True
        nx = self.vol.shape[0]
        ny, nz = self.masks[0]["segmentation"].shape
        self.ann_frame_idx = zSlice if zSlice is not None else nx // 2
        return self.propagate((nx, ny, nz))


    def generate_multi_slab(self, vol, thickness, zSlice):
        """tomo.py:141-158 ("highly experimental"): three slab projections a third of a slab apart as the three channels of one image,
        local contrast with a 3-sigma clip and one global min-max; kept as host glue (scipy's uniform_filter over all three axes, like
        the reference), it only sets self.image."""
        from scipy.ndimage import uniform_filter
        planes = [preprocess.project_tomogram(vol, zSlice + d, thickness) for d in (-thickness / 3, 0, thickness / 3)]
        image = np.stack(planes, axis=-1)
        mean = uniform_filter(image, size=500)
        var = np.clip(uniform_filter(image ** 2, size=500) - mean ** 2, a_min=0, a_max=None)
        image = np.clip((image - mean) / (np.sqrt(var) + 1e-8), -3, 3)
        self.image = preprocess.normalize(image, rgb=True)


class multiDepthTomoSegmenter(tomoSegmenter):
    """tomo.py:161-258: segment_vol seeded at num_slabs depths delta_z apart around the centre, binary union, 3-D connected components."""

    def __init__(self, deviceID: int = 0, cfg: Optional[AdapterConfig] = None, amg_cfg: Optional[cfgAMG] = None, target_class: int = 1,
                 min_mask_area: int = 100, min_rel_box_size: float = 0.025):
        self.min_rel_box_size = min_rel_box_size
        self.target_class = target_class
        super().__init__(deviceID=deviceID, cfg=cfg, amg_cfg=amg_cfg, min_mask_area=min_mask_area)
        if target_class < 1:
            raise ValueError("Multi-Depth Tomogram Segmenter only supports Single-Class Segmentation currently.")    # (the reference prints and exits)

    def segment(self, vol, thickness: int, num_slabs: int = 3, delta_z: int = 30, save_run: str = None, display: bool = False):
        self.show_segments = display
        if self.target_class > 0 or self.classifier is None:
            return self.single_segment(vol, thickness, num_slabs, delta_z)
        print("Multiclass Segmentation is not implemented yet")     # reference behaviour (tomo.py:201-203)

    @torch.inference_mode()
    def single_segment(self, vol, thickness, num_slabs, delta_z):
        from saber_amd.segmenters import utils
        depth = vol.shape[0]
        if self.device_volumes:          # the union stays on the device (csrc/labelvol.hip), so does the stitch; one download
            from saber_amd.utils import labelvol
            combined = torch.zeros(tuple(vol.shape), dtype=torch.int16, device=labelvol.require_device(self.device, "multiDepthTomoSegmenter with device_volumes"))
        else:
            combined = np.zeros(vol.shape, dtype=np.uint16)
        # the volume is prepared once for all slabs: every slab's set_volume then loads bit-equal frames, which is what lets the video
        # predictor keep its frame-feature store (SAM2AdapterConfig.frame_store_gb) from one slab to the next
        self._prepared = (vol, self.prepare_volume(vol))
        try:
            for i in range(num_slabs):
                centre = int(depth // 2 + (i - num_slabs // 2) * delta_z)
                if centre < 0 or centre >= depth:
                    print(f"Skipping slab {i}: slab_center={centre} out of range (0-{depth - 1})")
                    continue
                masks3d = self.segment_vol(vol, thickness, zSlice=centre, display=False)
                if masks3d is None:
                    continue
                if self.device_volumes:
                    labelvol.merge_max_u16_(combined, masks3d, binarize=True)
                else:
                    np.maximum(combined, (masks3d > 0).astype(np.uint16), out=combined)
        finally:
            self._prepared = None
        return self._stitch_device(combined) if self.device_volumes else utils.separate_masks(combined)
