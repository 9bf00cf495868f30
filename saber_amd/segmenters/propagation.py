"""propagationSegmenter (reference: saber/segmenters/propagation.py): volume segmenters for FIB / light / any
stack.  `slice_by_slice` (:163-189) is the volumetric hot loop this build accelerates: every z-slice is segmented
independently, painted into a uint16 label plane (idx+1, later masks overwrite), merged with np.maximum and the
stack is stitched by 3-D connected components.

Two implementations with identical results:
  * slice_by_slice           - the reference's loop shape over the adapter API (numpy dict lists at the edge);
  * slice_by_slice_device    - the device-resident, z-sharded form (saber_amd.segmenters.slice_driver): masks stay
                               bit-packed in HBM, label planes are painted by a HIP kernel and all-gathered over
                               RCCL when torch.distributed is initialised.
The seed-and-propagate entry points (segment / single_segment / multiclass_segment) run on the engine's video path
 and classifier (8f-3)."""
from typing import Optional

import numpy as np
import torch

from saber_amd.adapters.base import AdapterConfig
from saber_amd.adapters.sam2.amg import cfgAMG
from saber_amd.segmenters import utils
from saber_amd.segmenters.base import saber3D


class propagationSegmenter(saber3D):
    def __init__(self, deviceID: int = 0, cfg: Optional[AdapterConfig] = None, amg_cfg: Optional[cfgAMG] = None,
                 min_mask_area: int = 100, min_rel_box_size: float = 0.025):
        self.min_rel_box_size = min_rel_box_size
        super().__init__(deviceID=deviceID, cfg=cfg, amg_cfg=amg_cfg, min_mask_area=min_mask_area)
        self.ini_depth = 10

    @torch.inference_mode()
    def segment_3d(self, vol, masks, ann_frame_idx: int = None):
        if not self._vol_loaded:
            self.video_predictor.set_volume(vol)
            self._vol_loaded = True
        self.masks = masks
        nx = vol.shape[0]
        ny, nz = self.masks[0].shape[0], self.masks[0].shape[1]
        self.ann_frame_idx = ann_frame_idx if ann_frame_idx is not None else nx // 2
        return self.propagate((nx, ny, nz))

    def segment(self, volume: np.ndarray, ini_depth: int, nframes: int = None, target_class: int = 1,
                text_prompt: str = None, display: bool = False):
        self.ini_depth, self.nframes, self.target_class, self.display = ini_depth, nframes, target_class, display
        return self.single_segment(volume, text_prompt=text_prompt)

    @torch.inference_mode()
    def single_segment(self, volume: np.ndarray, text_prompt: str = None):
        if self.device_volumes:
            return self._single_segment_device(volume, text_prompt)
        final = np.zeros(volume.shape, dtype=np.uint16)
        for ii in range(2, volume.shape[0], self.ini_depth):
            masks = self.segment_image(volume[ii], display=False, target_class=self.target_class, text_prompt=text_prompt)
            if len(masks) == 0:
                continue
            masks3d = self.segment_3d(volume, [m["segmentation"] for m in masks], ann_frame_idx=ii)
            if self.target_class > 0:
                masks3d = (masks3d > 0).astype(np.uint8)
            np.maximum(final, masks3d, out=final)
        return utils.separate_masks(final)

    def _single_segment_device(self, volume, text_prompt):
        """single_segment with the union kept on the device: merge_max_u16 per seed slice (binarised exactly where the host loop
        binarises), the 3-D stitch on the device, one download"""
        from saber_amd.utils import labelvol
        dev = labelvol.require_device(self.device, "propagationSegmenter with device_volumes")
        final = torch.zeros(tuple(volume.shape), dtype=torch.int16, device=dev)
        for ii in range(2, volume.shape[0], self.ini_depth):
            masks = self.segment_image(volume[ii], display=False, target_class=self.target_class, text_prompt=text_prompt)
            if len(masks) == 0:
                continue
            masks3d = self.segment_3d(volume, [m["segmentation"] for m in masks], ann_frame_idx=ii)
            labelvol.merge_max_u16_(final, masks3d, binarize=self.target_class > 0)
        return self._stitch_device(final)

    @torch.inference_mode()
    def multiclass_segment(self, volume: np.ndarray):
        """propagation.py:119-160: per seed slice the raw 2-D masks are classified, the non-background ones propagated, and every voxel keeps
        the class of the most confident mask that reached it.  (The reference prepares the slice and hands the prepared RGB image to
        segment_image_2d, which prepares it again; kept.)"""
        from saber_amd.utils import preprocessing
        if self.device_volumes:
            from saber_amd.utils import labelvol, volprep
            dev = labelvol.require_device(self.device, "propagationSegmenter with device_volumes")
            final_dev = torch.zeros(tuple(volume.shape), dtype=torch.int16, device=dev)
            best_dev = torch.zeros(tuple(volume.shape), dtype=torch.float32, device=dev)
        else:
            final = np.zeros(volume.shape, dtype=np.uint16)
            best = np.zeros(volume.shape, dtype=np.float32)
        for ii in range(2, volume.shape[0], self.ini_depth):
            im = preprocessing.prepare(volume[ii], to_rgb=True)
            im = im.cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            gray = im[:, :, 0] if im.ndim == 3 else im
            raw = [m for m in self.adapter.segment_image_2d(np.repeat(gray[..., None], 3, axis=2)) if m["area"] >= self.min_mask_area]
            if len(raw) == 0:
                continue
            arrays = np.array([m["segmentation"].astype(np.uint8) for m in raw])
            predictions = self.classifier.batch_predict(gray, arrays, self.batchsize)
            classes = np.argmax(predictions, axis=1)
            valid = classes > 0
            if not np.any(valid):
                continue
            masks3d = self.segment_3d(volume, [raw[i]["segmentation"] for i, v in enumerate(valid) if v], ann_frame_idx=ii)
            if self.device_volumes:
                # the loop below as one pass: tables indexed by object id (idx + 1), entry 0 = background, never applied
                cids = classes[valid]
                cls = np.concatenate([[0], cids]).astype(np.uint16)
                conf = np.concatenate([[0], predictions[valid][np.arange(len(cids)), cids]]).astype(np.float32)
                labelvol.merge_class_conf_(final_dev, best_dev, masks3d, volprep.to_device_volume(cls, dev), torch.from_numpy(conf).to(dev))
                continue
            for idx, (probs, cid) in enumerate(zip(predictions[valid], classes[valid])):
                region = masks3d == (idx + 1)
                if np.any(region):
                    conf = probs[cid]
                    upd = region & (conf > best)
                    final[upd] = cid
                    best[upd] = conf
        if self.device_volumes:
            return final_dev.cpu().numpy().view(np.uint16)
        return final

    @torch.inference_mode()
    def slice_by_slice(self, volume: np.ndarray, text_prompt: str = None):
        """Independent 2-D segmentation of every slice, stitched in 3-D (reference :163-189)."""
        final = np.zeros(volume.shape, dtype=np.uint16)
        plane = np.zeros(volume.shape[1:], dtype=np.uint16)
        for z in range(volume.shape[0]):
            masks = self.segment_image(volume[z], display=False, text_prompt=text_prompt)
            if len(masks) == 0:
                continue
            for idx, m in enumerate(masks):
                plane[m["segmentation"]] = idx + 1
            np.maximum(final[z], plane, out=final[z])
            plane[:] = 0
        return utils.separate_masks(final)

    @torch.inference_mode()
    def slice_by_slice_device(self, volume, text_prompt: str = None, stitch: bool = True, handles_per_gpu: int = 2,
                              smooth_scale: float = None, sharded_stitch: bool = False, sharded_smooth: bool = False):
        """Same result as slice_by_slice, computed with device-resident masks and z-sharded over the ranks of the
        default torch.distributed process group (single process: all slices).  smooth_scale=0.05 appends the adaptive Gaussian
        smoothing segment_tomogram_core applies to the result (inference_core.py:68-74), still on the device (uint8 output).
        sharded_stitch: every rank labels its own z-chunk and the ranks exchange only what touches a seam (segment_volume_sharded); the
        result is the same volume on every rank.  sharded_smooth (with sharded_stitch and smooth_scale): every rank also smooths its own
        chunk from a few halo planes of its neighbours (segmenters/smooth.py) and the ranks gather the uint8 chunks; the same bytes."""
        from saber_amd.adapters.sam2.automask import get_replica
        from saber_amd.segmenters.slice_driver import segment_slice_to_plane, segment_volume_sharded
        gen = self.adapter._generator()
        eng, params = gen.base_generator.engine, gen.base_generator.params
        region_area = getattr(gen.base_generator, "min_mask_region_area", 0)       # the adapter's small-region clean-up, per slice
        hole_area, sprinkle_area = getattr(gen.base_generator, "max_hole_area", 0), getattr(gen.base_generator, "max_sprinkle_area", 0)
        engines = [eng]
        if handles_per_gpu > 1:
            # replicas of the PRIMARY engine's model (the adapter's own `cfg` field may name another trunk)
            engines += [get_replica(eng, r) for r in range(1, handles_per_gpu)]

        # classifier filter (saber2D._apply_classifier): one Predictor per thread, on an engine handle of its own.  When the classifier's
        # backbone IS the AMG engine, thread w's generator and classifier share replica w and run one after the other on that thread's
        # stream: the generator's masks and scalars are final (its call has synchronised) before the classifier's crops overwrite the
        # encoder slots.  self.batchsize lands in the component area filter, as on the host route (base.py, _apply_classifier).
        classifiers = [None] * len(engines)
        if self.classifier is not None:
            classifiers = [self.classifier if w == 0 else self.classifier.replica(get_replica(self.classifier.engine, w))
                           for w in range(len(engines))]

        def make(engine, classifier):
            def one(z):
                sl = volume[z]
                if isinstance(sl, np.ndarray):
                    sl = torch.from_numpy(np.ascontiguousarray(sl if sl.dtype == np.uint16 else sl.astype(np.float32))).to(engine.device)
                plane, _ = segment_slice_to_plane(engine, sl, params, min_mask_area=self.min_mask_area,
                                                  remove_repeating_masks=self.remove_repeating_masks, max_masks=gen.base_generator.max_masks,
                                                  classifier=classifier, target_class=1, classifier_min_area=self.batchsize,
                                                  **({"min_mask_region_area": region_area} if region_area > 0 else {}),
                                                  **({"max_hole_area": hole_area, "max_sprinkle_area": sprinkle_area}
                                                     if hole_area > 0 or sprinkle_area > 0 else {}))
                return plane
            return one

        one = [make(e, c) for e, c in zip(engines, classifiers)]
        if sharded_smooth and sharded_stitch and smooth_scale is not None:
            return segment_volume_sharded(volume, one, stitch=stitch, engine=eng, sharded_stitch=True, sharded_smooth=smooth_scale)
        return segment_volume_sharded(volume, one, stitch=stitch, engine=eng, smooth_scale=smooth_scale,   # 3-D CC (+ smoothing) on the device
                                      sharded_stitch=sharded_stitch)
