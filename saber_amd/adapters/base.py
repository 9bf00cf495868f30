"""Adapter ABC, configs and factory - the drop-in boundary of the hot path.

Mirrors saber/adapters/base.py of the reference: SAM2AdapterConfig (:7-33), BaseAdapter (:48-89),
get_adapter (:92-97).  Field names, defaults and validation errors are kept so that segmenters and CLI
code written against the reference work unchanged.
"""
from abc import ABC, abstractmethod
from typing import Any, Dict, Iterator, List, Literal, Optional, Tuple, Union

import numpy as np
from pydantic import BaseModel, ConfigDict, Field, field_validator, model_validator

_TRUNKS = {"tiny", "small", "base", "large"}


class SAM2AdapterConfig(BaseModel):
    model_config = ConfigDict(arbitrary_types_allowed=True)

    model_type: Literal["sam2"] = "sam2"
    cfg: str = Field("small", description="tiny / small / base / large")
    checkpoint: Optional[str] = None
    num_maskmem: int = 2
    # video path: background components of at most this many pixels of the tracked 256 x 256 mask logits are filled (upstream SAM2's
    # fill_hole_area; a default upstream build with its CUDA extension uses 8).  None -> SABER_AMD_FILL_HOLE_AREA, else 0 (off)
    fill_hole_area: Optional[int] = None
    # video path: GiB of device memory for the frame-feature store (16 MiB per frame: a frame of a volume goes through the encoder once,
    # whatever the number of seeds, directions and slabs).  None -> SABER_AMD_VIDEO_STORE_GB, else 0 (off)
    frame_store_gb: Optional[float] = None
    # video path: upstream SAM2's non_overlap_masks - at every pixel of the video-resolution logits a frame hands out, the object with the
    # highest logit (the first of them on a tie) keeps its value and the others are clamped to at most -10, so overlapping objects are
    # painted by confidence and not by paint order.  None -> SABER_AMD_NON_OVERLAP_MASKS=1, else off
    non_overlap_masks: Optional[bool] = None
    # mask generator: upstream's min_mask_region_area (postprocess_small_regions: holes and islands below that many pixels leave every
    # final mask, then a box NMS that prefers untouched masks), on the device.  None -> SABER_AMD_MIN_MASK_REGION_AREA, else 0 (off)
    min_mask_region_area: Optional[int] = None
    # mask generator: the predictor half of that upstream option (SAM2ImagePredictor(max_hole_area=A, max_sprinkle_area=A), which upstream's
    # generator builds for min_mask_region_area=A): background / foreground components of at most this many pixels of the 256 x 256 logits
    # are filled / removed before the masks are resized, thresholded and scored.  None -> SABER_AMD_MAX_HOLE_AREA / SABER_AMD_MAX_SPRINKLE_AREA,
    # else 0 (off); 0..65535.  An upstream build with its extension = all three options at A
    max_hole_area: Optional[int] = None
    max_sprinkle_area: Optional[int] = None
    light_modality: bool = False
    amg_cfg: Optional[Any] = None      # cfgAMG instance; None -> cfgAMG() defaults
    min_mask_area: int = 50
    classifier: Optional[Any] = None   # Predictor; fills cfg + amg_cfg from its config['amg_params']

    @model_validator(mode="after")
    def _derive_from_classifier(self) -> "SAM2AdapterConfig":
        if self.classifier is not None and self.amg_cfg is None:
            from saber_amd.adapters.sam2.amg import cfgAMG
            params = self.classifier.config["amg_params"]
            self.cfg = params.get("sam2_cfg", self.cfg)
            self.amg_cfg = cfgAMG(**params)
        return self

    @field_validator("cfg")
    @classmethod
    def _check_cfg(cls, v):
        if v not in _TRUNKS:
            raise ValueError(f"cfg must be one of tiny/small/base/large, got '{v}'")
        return v

    @field_validator("min_mask_region_area")
    @classmethod
    def _check_min_mask_region_area(cls, v):
        if v is not None and v < 0:
            raise ValueError("min_mask_region_area must be non-negative")
        return v

    @field_validator("max_hole_area", "max_sprinkle_area")
    @classmethod
    def _check_cleanup_area(cls, v, info):
        if v is not None and not 0 <= v <= 65535:
            raise ValueError(f"{info.field_name} must be from 0 to 65535")
        return v

    @field_validator("frame_store_gb")
    @classmethod
    def _check_frame_store_gb(cls, v):
        if v is not None and not v >= 0:
            raise ValueError("frame_store_gb must be non-negative")
        return v


class SAM3AdapterConfig(BaseModel):
    """Kept for signature compatibility; the SAM3 adapter is out of scope of this build."""
    model_type: Literal["sam3"] = "sam3"
    checkpoint_path: Optional[str] = None
    load_from_HF: bool = True
    light_modality: bool = False
    text_prompt: Optional[str] = None
    min_mask_area: int = 50


AdapterConfig = Union[SAM2AdapterConfig, SAM3AdapterConfig]


class BaseAdapter(ABC):
    """Common interface every tomogram adapter implements (reference: saber/adapters/base.py:48-89)."""

    frame_metrics: Dict[int, Dict[int, Dict[str, Any]]]

    @abstractmethod
    def segment_image_2d(self, image: np.ndarray, text_prompt: Optional[str] = None) -> List[Dict[str, Any]]:
        """2D segmentation; list of dicts with at least {'segmentation': (H,W) bool, 'area': int}."""

    @abstractmethod
    def set_volume(self, tomogram: np.ndarray, offload_video_to_cpu: bool = False) -> None: ...

    @abstractmethod
    def add_new_mask(self, frame_idx: int, obj_id: int, mask: np.ndarray, inference_state=None) -> Tuple: ...

    @abstractmethod
    def add_new_points_or_box(self, frame_idx: int, obj_id: int, inference_state=None, **kwargs) -> Tuple: ...

    @abstractmethod
    def propagate_in_video(self, start_frame_idx, max_frame_num_to_track=None, reverse=False, inference_state=None) -> Iterator: ...

    @abstractmethod
    def segment_volume(self, start_frame_idx: int, masks=None, vol_shape=None, max_frame_num_to_track=None,
                       min_presence_score: float = 0.5, inference_state=None) -> np.ndarray: ...

    @abstractmethod
    def reset_state(self, inference_state=None) -> None: ...


def get_adapter(config: AdapterConfig, device: str = "cuda") -> BaseAdapter:
    if config.model_type == "sam2":
        from saber_amd.adapters.sam2 import SAM2Adapter
        return SAM2Adapter(config, device)
    raise NotImplementedError("the SAM3 adapter is outside the MI355X hot-path build (SURVEY.md section 2 #19)")
