"""SAM2Adapter on the MI355X engine (reference: saber/adapters/sam2/predictor.py).

Hot-path method: segment_image_2d (:48-70) = prep.prepare -> lazily built mask generator -> generate.
The video-propagation methods of the ABC (set_volume / add_new_mask / propagate_in_video / segment_volume, :76-348) run the memory path
of saber_amd.adapters.sam2.video on a second engine handle built from config.cfg, like the reference's second model."""
import os
from typing import Any, Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch

from saber_amd.adapters.base import BaseAdapter, SAM2AdapterConfig
from saber_amd.adapters.sam2.amg import cfgAMG
from saber_amd.adapters.sam2.automask import build_amg
from saber_amd.utils import preprocessing as prep



class SAM2Adapter(BaseAdapter):
    def __init__(self, config: SAM2AdapterConfig, device="cuda"):
        if config.num_maskmem > 7:
            raise ValueError("num_maskmem must be at most 7")
        self._config = config
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        # the reference builds its video predictor from config.cfg here; that model belongs to the propagation path
        # (next row).  The AMG model is chosen by amg_cfg.sam2_cfg (automask.py:61) and is built lazily below.
        self.frame_metrics: Dict[int, Dict[int, Dict[str, Any]]] = {}
        self._vol_shape: Optional[Tuple[int, int, int]] = None
        self.inference_state = None
        self._mask_generator = None
        self._video_predictor = None

    def _generator(self):
        if self._mask_generator is None:
            if self._config.amg_cfg is not None:
                amg = self._config.amg_cfg.dict()
            else:
                amg = cfgAMG(sam2_cfg=self._config.cfg).dict()
            self._mask_generator = build_amg(amg, self._config.min_mask_area, device=self.device, checkpoint=self._config.checkpoint,
                                             min_mask_region_area=self._min_mask_region_area(), **self._lowres_cleanup())
        return self._mask_generator

    def _lowres_cleanup(self) -> Dict[str, int]:
        """config.max_hole_area / max_sprinkle_area, else the environment's SABER_AMD_MAX_HOLE_AREA / SABER_AMD_MAX_SPRINKLE_AREA, else 0 (off)"""
        from saber_amd.engine import lowres_cleanup_env_defaults
        cfg = (self._config.max_hole_area, self._config.max_sprinkle_area)
        env = lowres_cleanup_env_defaults() if None in cfg else (0, 0)
        h, s = (int(c) if c is not None else e for c, e in zip(cfg, env))
        return {"max_hole_area": h, "max_sprinkle_area": s}

    def _min_mask_region_area(self) -> int:
        """config.min_mask_region_area, else the environment's SABER_AMD_MIN_MASK_REGION_AREA, else 0 (off, upstream's default)"""
        if self._config.min_mask_region_area is not None:
            v = int(self._config.min_mask_region_area)
        else:
            v = int(os.environ.get("SABER_AMD_MIN_MASK_REGION_AREA") or 0)
        if v < 0:
            raise ValueError("min_mask_region_area must be non-negative")
        return v

    @property
    def engine(self):
        return self._generator().base_generator.engine

    @torch.inference_mode()
    def segment_image_2d(self, image: np.ndarray, text_prompt: str = None, threshold: float = None) -> List[Dict[str, Any]]:
        """(H,W) gray or (H,W,3) image of any float range -> SAM-AMG dict list (caller owns the arrays)."""
        gen = self._generator()
        if image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3):
            raise ValueError(f"segment_image_2d: expected (H,W) or (H,W,3), got {image.shape}")
        # (H,W): gray slice, the reference repeats it to 3 channels (to_rgb=True).  (H,W,3): the reference passes the array
        # through prepare(to_rgb=False): box filter over all three axes, one global min/max (predictor.py:58-59)
        img = prep.prepare(image, to_rgb=image.ndim == 2, engine=gen.base_generator.engine)
        return gen.generate(img)

    # ------------------------------------------------------------------ video path
    def _video(self):
        """The video predictor shares the trunk named by config.cfg (reference predictor.py:21-26 builds it from config.cfg, the AMG model
        from amg_cfg.sam2_cfg - two models, as in the reference)."""
        if self._video_predictor is None:
            from saber_amd import pretrained_weights
            from saber_amd.adapters.sam2.automask import get_engine
            from saber_amd.adapters.sam2.video import VideoPredictor
            # max_images = frames per batched encoder pass of the tracking loop (VideoPredictor._frame); multipoint: add_new_points_or_box with a
            # box or several clicks runs on the handle's 16-bit decoder kernels (16-token route)
            eng = get_engine(self._config.cfg, self.device, self._config.checkpoint, max_images=16, max_prompts=8, replica=1000, multipoint=True)
            W = pretrained_weights.load_weights(self._config.cfg, self._config.checkpoint, video=True)
            self._video_predictor = VideoPredictor(eng, W, num_maskmem=self._config.num_maskmem, fill_hole_area=self._fill_hole_area(),
                                                   frame_store_gb=self._config.frame_store_gb, non_overlap_masks=self._config.non_overlap_masks)
        return self._video_predictor

    def _fill_hole_area(self) -> int:
        """config.fill_hole_area, else the environment's SABER_AMD_FILL_HOLE_AREA, else 0 (off; upstream's default build fills holes of up to 8)"""
        if self._config.fill_hole_area is not None:
            return int(self._config.fill_hole_area)
        return int(os.environ.get("SABER_AMD_FILL_HOLE_AREA") or 0)

    @torch.inference_mode()
    def set_volume(self, tomogram, offload_video_to_cpu: bool = False) -> None:
        """predictor.py:76-86: normalise the tomogram, resize every slice to the model's 1024^2, start an empty inference state.
        tomogram: (Z,H,W) numpy, or a CUDA float32 tensor, which is used where it lies"""
        from saber_amd.adapters.sam2.video import load_tomogram_frames_device
        self._vol_shape = tuple(tomogram.shape)
        self.frame_metrics = {}
        vp = self._video()
        frames = load_tomogram_frames_device(tomogram, vp.lib, vp.dev, 1024, self._config.light_modality)
        vp.init_state(frames, video_hw=(1024, 1024))            # the reference reports the RESIZED size as the video size (preprocessing.py:24)
        self.inference_state = vp

    def add_new_mask(self, frame_idx: int, obj_id: int, mask: np.ndarray, inference_state=None) -> Tuple:
        state = inference_state or self.inference_state
        if state is None:
            raise RuntimeError("Call set_volume() before add_new_mask().")
        return state.add_new_mask(frame_idx, obj_id, mask)

    def add_new_points_or_box(self, frame_idx: int, obj_id: int, inference_state=None, **kwargs) -> Tuple:
        """predictor.py:171-180: delegates to the video predictor (points=, labels=, clear_old_points=, normalize_coords=, box=).  Clicks,
        several clicks per call, boxes and corrections of tracked frames follow upstream (adapters/sam2/video.py); prompts of more than one
        point are decoded on the handle's 16-bit kernels (the 16-token route: _video() builds its handle with multipoint on).  No SABER
        caller uses them: segmenters/base.py:265-280 seeds propagation with masks."""
        state = inference_state or self.inference_state
        if state is None:
            raise RuntimeError("Call set_volume() before add_new_points_or_box().")
        return state.add_new_points_or_box(frame_idx, obj_id, **kwargs)

    @torch.inference_mode()
    def propagate_in_video(self, start_frame_idx, max_frame_num_to_track=None, reverse=False, inference_state=None) -> Iterator:
        """yields (frame_idx, obj_ids, mask_logits, mask_logits, None) like the reference (predictor.py:181-202)"""
        state = inference_state or self.inference_state
        if state is None:
            raise RuntimeError("Call set_volume() before propagate_in_video().")
        for t, ids, logits in state.propagate_in_video(start_frame_idx, max_frame_num_to_track, reverse):
            yield t, ids, logits, logits, None

    @staticmethod
    def _normalize_masks(masks) -> List[np.ndarray]:
        if masks is None:
            return []
        if isinstance(masks, torch.Tensor):
            masks = masks.cpu().numpy()
        if isinstance(masks, np.ndarray) and masks.ndim >= 3:
            return [np.squeeze(masks[i]).astype(np.float32) for i in range(masks.shape[0])]
        out = []
        for m in masks:
            if isinstance(m, torch.Tensor):
                m = m.cpu().numpy()
            if isinstance(m, dict):
                m = m["segmentation"]
            out.append(np.squeeze(m).astype(np.float32))
        return out

    @torch.inference_mode()
    def segment_volume(self, start_frame_idx: int, masks=None, vol_shape=None, max_frame_num_to_track=None,
                       min_presence_score: float = 0.5, inference_state=None, *, device_volume: bool = False,
                       batch_objects: Optional[bool] = None, non_overlap_masks: Optional[bool] = None):
        """Bidirectional propagation + presence-score filter, predictor.py:232-348 step by step.  The reference captures the mask decoder's
        object-score logits with a forward hook and files them under `_current_frame`, which it updates only AFTER the generator has
        yielded a frame: a frame's scores therefore land on the frame yielded before it.  Reproduced as is (it feeds the boundary fit).
        device_volume=True: the same label volume stays on the device (saber_amd/utils/labelvol.py, csrc/labelvol.hip) - one paint launch
        per frame for all its objects, the presence filter as one (Z, n + 1) table look-up - and comes back as the (Z,H,W) int16 tensor
        of uint16 values Engine.separate_masks accepts; frame_metrics and frame_scores are filled as on the host route.
        batch_objects=True / False: the memory attention of all objects of a frame as one set of launches, or object by object, for this
        call (VideoPredictor.batch_objects; same bits either way); None keeps the video predictor's own setting (SABER_AMD_VIDEO_BATCH).
        non_overlap_masks=True / False: upstream's option of that name for this call (VideoPredictor.non_overlap_masks): the yielded logits
        have at most one object above -10 at a pixel, so where seeds or tracked masks overlap the voxel gets the id of the object with the
        highest logit (the lowest id on a tie, as on the seeded frame, where seeds tie at +10) instead of the highest id painted last;
        frame_scores and everything the tracker stores are the same.  None keeps the predictor's own setting (SAM2AdapterConfig /
        SABER_AMD_NON_OVERLAP_MASKS)."""
        from saber_amd.filters.estimate_thickness import fit_organelle_boundaries
        if device_volume:
            from saber_amd.utils import labelvol, volprep
            labelvol.require_device(self.device, "SAM2Adapter.segment_volume(device_volume=True)")
        state = inference_state or self.inference_state
        if state is None:
            raise RuntimeError("Call set_volume() before segment_volume().")
        if vol_shape is None:
            vol_shape = self._vol_shape
        if vol_shape is None:
            raise RuntimeError("vol_shape required when inference_state is passed explicitly.")
        Z, H, W = vol_shape
        mask_list = self._normalize_masks(masks)
        current = {"frame": None}
        captured: Dict[Any, list] = {}
        state.hook = lambda score: captured.setdefault(current["frame"], []).append(np.array([score], dtype=np.float32))
        was_batched = state.batch_objects
        if batch_objects is not None:
            state.batch_objects = bool(batch_objects)
        was_non_overlap = state.non_overlap_masks
        if non_overlap_masks is not None:
            state.non_overlap_masks = bool(non_overlap_masks)
        try:
            for obj_id, mask in enumerate(mask_list, start=1):
                if np.max(mask) == 0:
                    continue
                self.add_new_mask(frame_idx=start_frame_idx, obj_id=obj_id, mask=mask, inference_state=state)
            self.frame_metrics = {}
            # the label volume is painted on the device (threshold + nearest resize to the tomogram's size + label, one launch per object
            # and frame) and comes back to the host once, after both passes
            import ctypes as C
            vol_dev = torch.zeros((Z, H, W), dtype=torch.int16, device=state.dev)
            flag = torch.zeros(1, dtype=torch.int32, device=state.dev)
            painted = set()

            def _apply(frame_idx, obj_ids, mask_logits, want_flag=False):
                Hv, Wv = mask_logits.shape[-2:]
                stream = C.c_void_p(torch.cuda.current_stream(state.dev).cuda_stream)
                for i, obj_id in enumerate(obj_ids):
                    lg = mask_logits[i, 0]
                    if state.lib.saber_k_paint_nearest(C.c_void_p(lg.data_ptr()), Hv, Wv, 0.0, int(obj_id), C.c_void_p(vol_dev[frame_idx].data_ptr()), H, W,
                                                       C.c_void_p(flag.data_ptr()) if want_flag else None, stream) != 0:
                        raise RuntimeError(state.lib.saber_k_last_error().decode())
                painted.add(frame_idx)

            def _apply_stack(frame_idx, obj_ids, mask_logits, want_flag=False):
                labelvol.paint_nearest_stack(mask_logits, obj_ids, vol_dev[frame_idx], 0.0, flag if want_flag else None)
                painted.add(frame_idx)

            if device_volume:
                _apply = _apply_stack
            for frame_idx, obj_ids, mask_logits, _, _ in self.propagate_in_video(start_frame_idx, max_frame_num_to_track, False, state):
                current["frame"] = frame_idx
                _apply(frame_idx, obj_ids, mask_logits, want_flag=(frame_idx == start_frame_idx))
            for frame_idx, obj_ids, mask_logits, _, _ in self.propagate_in_video(start_frame_idx, max_frame_num_to_track, True, state):
                current["frame"] = frame_idx
                # predictor.py:318-319: only frames the forward pass left empty.  Both passes share the start frame alone; whether its
                # forward masks painted a pixel is the one thing read back here
                if frame_idx not in painted or (frame_idx == start_frame_idx and int(flag.item()) == 0):
                    _apply(frame_idx, obj_ids, mask_logits)
            vol_masks = None if device_volume else vol_dev.cpu().numpy().view(np.uint16)
        finally:
            state.hook = None
            state.batch_objects = was_batched
            state.non_overlap_masks = was_non_overlap
        n_masks = len(mask_list)
        if n_masks > 0:
            frame_scores = np.zeros([Z, n_masks])
            for fidx, scores in captured.items():
                if fidx is None:
                    continue
                v = np.concatenate([s.flatten() for s in scores])
                n = min(len(v), n_masks)
                frame_scores[fidx, :n] = v[:n]
            self.frame_scores = frame_scores
            bounds = fit_organelle_boundaries(frame_scores, plot=False)
            if device_volume:          # the filter below as one table, uploaded once: nothing of volume size crosses to the host
                labelvol.relabel_frames_(vol_dev, volprep.to_device_volume(labelvol.presence_keep_table(bounds, min_presence_score), vol_dev.device))
            for fidx in range(Z):
                self.frame_metrics[fidx] = {}
                for mi in range(n_masks):
                    obj_id = mi + 1
                    ps = float(bounds[fidx, mi])
                    self.frame_metrics[fidx][obj_id] = {"presence_score": ps}
                    if ps < min_presence_score and not device_volume:
                        vol_masks[fidx][vol_masks[fidx] == obj_id] = 0
        if device_volume:
            return vol_dev
        return vol_masks.astype(np.uint16)

    def clear_all_prompts_in_frame(self, *args, inference_state=None, **kwargs):
        """predictor.py:360-362: delegates to the video predictor (frame_idx, obj_id, need_output=True).  The reference passes upstream's
        inference_state as the first positional argument; here the state IS the predictor, so a leading state object is dropped."""
        state = inference_state or self.inference_state
        if args and hasattr(args[0], "clear_all_prompts_in_frame"):
            state, args = args[0], args[1:]
        if state is None:
            raise RuntimeError("Call set_volume() before clear_all_prompts_in_frame().")
        return state.clear_all_prompts_in_frame(*args, **kwargs)

    def remove_object(self, *args, inference_state=None, **kwargs):
        """predictor.py:364-366: delegates to the video predictor (obj_id, strict=False, need_output=True)."""
        state = inference_state or self.inference_state
        if args and hasattr(args[0], "remove_object"):
            state, args = args[0], args[1:]
        if state is None:
            raise RuntimeError("Call set_volume() before remove_object().")
        return state.remove_object(*args, **kwargs)

    def reset_state(self, inference_state=None) -> None:
        state = inference_state or self.inference_state
        if state is not None:
            state.reset_state()          # like upstream's reset_state: prompts and tracking results go, the loaded frames stay
