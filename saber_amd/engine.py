"""Python host wrapper of the C-ABI engine: PyTorch-ROCm tensors in, masks out.

PyTorch is used only for device memory, streams and (elsewhere) torch.distributed; every
arithmetic step of the hot path runs in the HIP library.  Errors from the C-ABI surface as
Python exceptions (ValueError for bad configuration, RuntimeError for state / HIP errors) so
that the reference's per-task accounting (saber/utils/parallelization.py:129-135) keeps working.
"""
import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .model_config import get_config
from .weights import seeded_weights, load_checkpoint

SABER_U16, SABER_F32 = 0, 1


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Engine:
    """One engine handle bound to one device (reference threading contract: one caller per device)."""

    def __init__(self, trunk: str = "large", device: int = 0, weights: Optional[Dict[str, np.ndarray]] = None,
                 checkpoint: Optional[str] = None, seed: int = 0, max_images: int = 1, max_prompts: int = 64, weight_format: str = "bf16", precision: str = "bf16",
                 operands: Optional[str] = None, multipoint: bool = False):
        self.lib = _lib.load()
        self.cfg = get_config(trunk)  # ValueError for unknown names, like the reference
        if not torch.cuda.is_available():
            raise RuntimeError("saber_amd.Engine needs a ROCm device (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device(f"cuda:{device}")
        self.device_index = device
        h = C.c_void_p()
        st = self.lib.saber_engine_create(device, trunk.encode(), max_images, max_prompts, C.byref(h))
        if st != 0:
            msg = self.lib.saber_last_error(None).decode()
            raise (ValueError if st == -1 else RuntimeError)(msg)
        self.h = h
        self.max_images, self.max_prompts = max_images, max_prompts
        if weight_format not in ("bf16", "fp8", "mxfp8"):
            raise ValueError(f"weight_format must be 'bf16', 'fp8' or 'mxfp8', got '{weight_format}'")
        self.weight_format = weight_format
        if weight_format != "bf16":      # fp8: e4m3 storage of the stage-2/3 block weights; mxfp8: MX operands on the fp8 MFMA (include/saber_amd.h: saber_engine_set_weight_format)
            self._check(self.lib.saber_engine_set_weight_format(self.h, {"fp8": 1, "mxfp8": 2}[weight_format]))
        if precision not in ("bf16", "fp16", "exact"):
            raise ValueError(f"precision must be 'bf16', 'fp16' or 'exact', got '{precision}'")
        # operands: the 16-bit MFMA operand type the weights are converted to at finalize ("bf16" | "fp16"; include/saber_amd.h:
        # SABER_PRECISION_FP16).  Implied by `precision`; only a handle created with precision="exact" needs it spelled out, to say which
        # 16-bit arithmetic set_precision can switch back to.
        if operands is None:
            operands = "fp16" if precision == "fp16" else "bf16"
        if operands not in ("bf16", "fp16") or (precision in ("bf16", "fp16") and operands != precision):
            raise ValueError(f"operands must be 'bf16' or 'fp16' and agree with precision, got operands='{operands}' precision='{precision}'")
        self.operands = operands
        self.precision = precision
        self.has_exact = precision == "exact"      # fp32 weight copies are kept only when the handle was created in the exact mode
        if operands == "fp16":
            self._check(self.lib.saber_engine_set_precision(self.h, 2))
        if precision == "exact":         # fp32 operands everywhere (include/saber_amd.h: saber_engine_set_precision); keeps fp32 weight copies
            self._check(self.lib.saber_engine_set_precision(self.h, 1))
        self.multipoint = False
        if multipoint:
            self.set_multipoint(True)
        if weights is None:
            weights = load_checkpoint(checkpoint, self.cfg) if checkpoint else seeded_weights(self.cfg, seed)
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            self._check(self.lib.saber_engine_set_weight(self.h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))
        self._check(self.lib.saber_engine_finalize(self.h))

    @classmethod
    def bare(cls, device: int = 0) -> "Engine":
        """A handle without model weights: enough for the volume post-processing calls (separate_masks, smooth_labels,
        gaussian_smoothing_3d), which only need the device binding and the per-handle error string."""
        self = cls.__new__(cls)
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("saber_amd.Engine needs a ROCm device (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device(f"cuda:{device}")
        self.device_index = device
        h = C.c_void_p()
        st = self.lib.saber_engine_create(device, b"tiny", 1, 1, C.byref(h))
        if st != 0:
            raise RuntimeError(self.lib.saber_last_error(None).decode())
        self.h = h
        self.cfg = None
        self.max_images = self.max_prompts = 0
        self.multipoint = False
        return self

    def _check(self, st: int):
        if st != 0:
            msg = self.lib.saber_last_error(self.h).decode()
            raise (ValueError if st == -1 else _lib.SaberRangeError if st == _lib.SABER_ERR_RANGE else RuntimeError)(f"saber_amd: {msg}")

    def check_finite(self):
        """Overflow sentinel (include/saber_amd.h: saber_engine_check_finite): waits for the current stream and raises SaberRangeError when an
        encode / decode since the last check produced NaN / inf (fp16 operands: an activation beyond 65 504).  amg_generate checks by itself;
        call this after encode / decode_points where the host synchronises anyway."""
        self._check(self.lib.saber_engine_check_finite(self.h, _stream()))

    def close(self):
        if getattr(self, "h", None):
            self.lib.saber_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ K0
    def prepare(self, img: torch.Tensor) -> torch.Tensor:
        """prep.prepare on device.  img: (H,W) uint16 or float32 device tensor -> (H,W) float32 in [0,1];
        (H,W,3) float32 -> (H,W,3) float32 (the reference's treatment of an RGB array: box filter over all three axes, one min/max)."""
        assert img.is_cuda and img.is_contiguous()
        if img.dim() == 3:
            if img.shape[2] != 3 or img.dtype != torch.float32:
                raise ValueError(f"prepare: a 3-D input must be (H,W,3) float32, got {tuple(img.shape)} {img.dtype}")
            out = torch.empty(img.shape, dtype=torch.float32, device=img.device)
            self._check(self.lib.saber_prepare_rgb(self.h, _ptr(img), img.shape[0], img.shape[1], _ptr(out), _stream()))
            return out
        assert img.dim() == 2
        if img.dtype == torch.uint16:
            dt = SABER_U16
        elif img.dtype == torch.float32:
            dt = SABER_F32
        else:
            raise ValueError(f"prepare: unsupported dtype {img.dtype}")
        out = torch.empty(img.shape, dtype=torch.float32, device=img.device)
        self._check(self.lib.saber_prepare(self.h, _ptr(img), dt, img.shape[0], img.shape[1], _ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ encoder
    def encode(self, img: torch.Tensor, crop_boxes: Optional[Sequence[Sequence[int]]] = None, slot0: int = 0, normalised_grey: bool = False):
        """img: (H,W) or (H,W,3) float32 in [0,1] on the device; crop_boxes: list of [x0,y0,x1,y1].  normalised_grey: (H,W) plane that
        already carries the model's input normalisation (channels = -1 of saber_encode)."""
        assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous()
        H, W = img.shape[:2]
        ch = 1 if img.dim() == 2 else img.shape[2]
        if normalised_grey:
            assert img.dim() == 2
            ch = -1
        if crop_boxes is None:
            crop_boxes = [[0, 0, W, H]]
        cb = np.ascontiguousarray(np.asarray(crop_boxes, dtype=np.int32).reshape(-1, 4))
        self._check(self.lib.saber_encode(self.h, _ptr(img), H, W, ch, cb.ctypes.data_as(C.POINTER(C.c_int)), len(cb), slot0, _stream()))

    def get_features(self, slot: int = 0):
        emb = torch.empty((256, 64, 64), dtype=torch.float32, device=self.device)
        s0 = torch.empty((32, 256, 256), dtype=torch.float32, device=self.device)
        s1 = torch.empty((64, 128, 128), dtype=torch.float32, device=self.device)
        self._check(self.lib.saber_get_features(self.h, slot, _ptr(emb), _ptr(s0), _ptr(s1), _stream()))
        return {"image_embed": emb, "feat_s0": s0, "feat_s1": s1}

    # ------------------------------------------------------------------ decoder
    def decode_points(self, pts: torch.Tensor, slot: int = 0, multimask: bool = True, mask_input: Optional[torch.Tensor] = None,
                      labels: Optional[torch.Tensor] = None):
        """pts: (n,2) float32 model-pixel coords on device. Returns (lowres (n,M,256,256), iou (n,M), obj (n,))."""
        assert pts.is_cuda and pts.dtype == torch.float32 and pts.is_contiguous()
        n = pts.shape[0]
        M = 3 if multimask else 1
        low = torch.empty((n, M, 256, 256), dtype=torch.float32, device=self.device)
        iou = torch.empty((n, M), dtype=torch.float32, device=self.device)
        obj = torch.empty((n,), dtype=torch.float32, device=self.device)
        if mask_input is not None:
            assert mask_input.is_cuda and mask_input.dtype == torch.float32 and mask_input.is_contiguous() and mask_input.numel() == n * 65536
        if labels is not None:
            assert labels.is_cuda and labels.dtype == torch.int32 and labels.numel() == n
        self._check(self.lib.saber_decode_points(self.h, slot, _ptr(pts), _ptr(labels), n, int(multimask), _ptr(mask_input),
                                                 _ptr(low), _ptr(iou), _ptr(obj), _stream()))
        return low, iou, obj

    def decode_prompts(self, pts: torch.Tensor, labels: torch.Tensor, slot: int = 0, multimask: bool = False, mask_input: Optional[torch.Tensor] = None):
        """Prompts of several points each (clicks with labels 1 / 0; a box = its two corners with labels 2 / 3 first; -1 = not a point).
        pts: (n,k,2) float32 model-pixel coords, labels: (n,k) int32, both on the device, k = 1..9.  With k > 1 the handle must be in the
        exact precision mode, or have multipoint on (set_multipoint: the 16-token route of the 16-bit decoder kernels, chunks of
        max_prompts / 2 prompts); otherwise RuntimeError.  Returns (lowres (n,M,256,256), iou (n,M), obj (n,))."""
        assert pts.is_cuda and pts.dtype == torch.float32 and pts.is_contiguous() and pts.dim() == 3 and pts.shape[2] == 2
        n, k = pts.shape[:2]
        assert labels.is_cuda and labels.dtype == torch.int32 and labels.is_contiguous() and tuple(labels.shape) == (n, k)
        M = 3 if multimask else 1
        low = torch.empty((n, M, 256, 256), dtype=torch.float32, device=self.device)
        iou = torch.empty((n, M), dtype=torch.float32, device=self.device)
        obj = torch.empty((n,), dtype=torch.float32, device=self.device)
        if mask_input is not None:
            assert mask_input.is_cuda and mask_input.dtype == torch.float32 and mask_input.is_contiguous() and mask_input.numel() == n * 65536
        self._check(self.lib.saber_decode_prompts(self.h, slot, _ptr(pts), _ptr(labels), n, k, int(multimask), _ptr(mask_input),
                                                  _ptr(low), _ptr(iou), _ptr(obj), _stream()))
        return low, iou, obj

    # ------------------------------------------------------------------ AMG
    def amg_generate(self, img: torch.Tensor, params: "_lib.AmgParams", max_masks: int = 1024, min_mask_region_area: int = 0,
                     max_hole_area: int = 0, max_sprinkle_area: int = 0):
        """img: (H,W) or (H,W,3) float32 in [0,1].  Returns (bits uint32 (n,H,W32) device tensor, list of MaskMeta).
        min_mask_region_area > 0: upstream's option of that name - postprocess_small_regions on the final masks with the NMS threshold
        max(params.box_nms_thresh, params.crop_nms_thresh); 0 (default) = off: no launch, nothing allocated.
        max_hole_area / max_sprinkle_area > 0: the predictor half of that upstream option for this call (set_lowres_cleanup; the handle's
        own setting is back afterwards); 0 / 0 (default) = the handle's setting, which is off unless set_lowres_cleanup was called.  An
        upstream generator built with its connected-components extension equals min_mask_region_area=A, max_hole_area=A, max_sprinkle_area=A."""
        if min_mask_region_area < 0:
            raise ValueError("min_mask_region_area must be non-negative")
        _check_cleanup_areas("amg_generate", max_hole_area, max_sprinkle_area)
        if max_hole_area or max_sprinkle_area:
            keep = getattr(self, "_lowres_cleanup", (0, 0))
            self.set_lowres_cleanup(max_hole_area, max_sprinkle_area)
            try:
                return self.amg_generate(img, params, max_masks=max_masks, min_mask_region_area=min_mask_region_area)
            finally:
                self.set_lowres_cleanup(*keep)
        if min_mask_region_area > 0:
            bits, meta = self.amg_generate(img, params, max_masks=max_masks)
            return self.postprocess_small_regions(bits, meta, img.shape[0], img.shape[1], min_mask_region_area,
                                                  max(params.box_nms_thresh, params.crop_nms_thresh))
        assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous()
        H, W = img.shape[:2]
        ch = 1 if img.dim() == 2 else img.shape[2]
        W32 = (W + 31) // 32
        bits = torch.empty((max_masks, H, W32), dtype=torch.int32, device=self.device)
        meta = (_lib.MaskMeta * max_masks)()
        cnt = C.c_int(0)
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream == 0:
            # hipGraph capture is not possible on the legacy default stream: run on a stream of this handle, ordered after / before it
            side = getattr(self, "_side_stream", None)
            if side is None:
                side = self._side_stream = torch.cuda.Stream(self.device)
            side.wait_stream(cur)
            st = self.lib.saber_amg_generate(self.h, _ptr(img), H, W, ch, C.byref(params), _ptr(bits), max_masks, meta, C.byref(cnt), C.c_void_p(side.cuda_stream))
            cur.wait_stream(side)
        else:
            st = self.lib.saber_amg_generate(self.h, _ptr(img), H, W, ch, C.byref(params), _ptr(bits), max_masks, meta, C.byref(cnt), _stream())
        if st == _lib.SABER_ERR_CAPACITY and cnt.value > max_masks:
            # the engine reports the count it needed: retry once with that capacity instead of failing the slice
            return self.amg_generate(img, params, max_masks=cnt.value)
        self._check(st)
        n = cnt.value
        return bits[:n], [meta[i] for i in range(n)]

    # ------------------------------------------------------------------ low-res clean-up (csrc/lowres_cleanup.hip)
    def clean_lowres(self, planes: torch.Tensor, max_hole_area: int, max_sprinkle_area: int, mask_threshold: float = 0.0) -> torch.Tensor:
        """Upstream's SAM2Transforms.postprocess_masks on an (n,H,W) float32 device tensor of mask logits, IN PLACE (include/saber_amd_kernels.h:
        saber_k_clean_lowres): per plane, 8-connected background components (x <= mask_threshold) of at most max_hole_area pixels become
        mask_threshold + 10, foreground components of at most max_sprinkle_area pixels mask_threshold - 10, both found on the original
        values.  H * W <= 65536, areas 0..65535 (0 = that half off).  Returns `planes`.  One launch, no host synchronisation."""
        if not torch.cuda.is_available():
            raise RuntimeError("saber_amd.Engine.clean_lowres needs a ROCm device; there is no CPU fallback")
        if not isinstance(planes, torch.Tensor) or not planes.is_cuda or planes.dtype != torch.float32 or planes.dim() != 3 or not planes.is_contiguous():
            raise ValueError("clean_lowres: planes must be a contiguous (n,H,W) float32 device tensor")
        if planes.device != self.device:
            raise ValueError(f"clean_lowres: the planes are on {planes.device}, the engine on {self.device}")
        _check_cleanup_areas("clean_lowres", max_hole_area, max_sprinkle_area)
        n, H, W = (int(v) for v in planes.shape)
        if n == 0:
            return planes
        with torch.cuda.device(self.device):
            if self.lib.saber_k_clean_lowres(_ptr(planes), None, None, n, H, W, float(mask_threshold), int(max_hole_area), int(max_sprinkle_area), _stream()) != 0:
                raise ValueError(f"saber_amd: {self.lib.saber_k_last_error().decode()}")
        return planes

    def set_lowres_cleanup(self, max_hole_area: int, max_sprinkle_area: int):
        """The predictor half of upstream's min_mask_region_area in amg_generate (include/saber_amd.h: saber_engine_set_lowres_cleanup): the
        low-res planes the masks are made from are cleaned before they are resized, thresholded and scored.  0, 0 (default) = off."""
        _check_cleanup_areas("set_lowres_cleanup", max_hole_area, max_sprinkle_area)
        self._check(self.lib.saber_engine_set_lowres_cleanup(self.h, int(max_hole_area), int(max_sprinkle_area)))
        self._lowres_cleanup = (int(max_hole_area), int(max_sprinkle_area))

    # ------------------------------------------------------------------ small regions (csrc/smallregions.hip)
    SMALL_REGIONS_WS_BYTES = 128 << 20      # label workspace of remove_small_regions: the masks are run in passes of as many as it holds

    def _check_packed(self, who: str, bits, W: int):
        if not isinstance(bits, torch.Tensor) or not bits.is_cuda:
            raise ValueError(f"{who}: the mask stack must be a device tensor")
        if bits.dtype not in (torch.int32, torch.uint32) or bits.dim() != 3 or bits.shape[2] != (int(W) + 31) // 32 or int(W) < 1:
            raise ValueError(f"{who}: the mask stack must be (n,H,ceil(W/32)) int32 for W = {W}, got {tuple(bits.shape)} {bits.dtype}")
        if bits.device != self.device:
            raise ValueError(f"{who}: the mask stack is on {bits.device}, the engine on {self.device}")
        return bits.contiguous()

    def remove_small_regions(self, bits: torch.Tensor, W: int, min_area: int):
        """Holes, then islands, of fewer than min_area pixels (8-connected) of every mask of a bit-packed (n,H,W32) int32 device stack
        (include/saber_amd_kernels.h: saber_k_mask_small_regions).  Returns device tensors (bits_out (n,H,W32), changed (n,) int32 0/1,
        area (n,) int32, boxes (n,4) int32 [x0,y0,x1,y1] with inclusive maxima); the input is left as it is.  No host synchronisation."""
        if not torch.cuda.is_available():
            raise RuntimeError("saber_amd.Engine.remove_small_regions needs a ROCm device; there is no CPU fallback")
        bits = self._check_packed("remove_small_regions", bits, W)
        if min_area < 1:
            raise ValueError("remove_small_regions: min_area must be at least 1")
        n, H = int(bits.shape[0]), int(bits.shape[1])
        out = torch.empty_like(bits)
        changed = torch.empty((n,), dtype=torch.int32, device=self.device)
        area = torch.empty((n,), dtype=torch.int32, device=self.device)
        boxes = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        if n == 0 or H == 0:
            return out, changed, area, boxes
        per = int(self.lib.saber_k_mask_small_regions_bytes(H, int(W)))
        ws = torch.empty((per * max(1, min(n, self.SMALL_REGIONS_WS_BYTES // per)),), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            if self.lib.saber_k_mask_small_regions(_ptr(bits), n, H, int(W), int(min_area), _ptr(out), _ptr(changed), _ptr(area), _ptr(boxes), _ptr(ws),
                                                   ws.numel(), _stream()) != 0:
                raise ValueError(f"saber_amd: {self.lib.saber_k_last_error().decode()}")
        return out, changed, area, boxes

    def postprocess_small_regions(self, bits: torch.Tensor, meta, H: int, W: int, min_area: int, nms_thresh: float):
        """SAM2AutomaticMaskGenerator.postprocess_small_regions on what amg_generate returned (include/saber_amd.h:
        saber_amg_postprocess_small_regions): small holes filled and small islands removed per mask, box NMS that prefers untouched
        masks, survivors in NMS order.  bits: (n,H,W32) int32 device tensor, meta: its n MaskMeta records.  Returns (bits, meta) like
        amg_generate; the inputs are left as they are.  One host synchronisation."""
        if not torch.cuda.is_available():
            raise RuntimeError("saber_amd.Engine.postprocess_small_regions needs a ROCm device; there is no CPU fallback")
        bits = self._check_packed("postprocess_small_regions", bits, W)
        n = int(bits.shape[0])
        if len(meta) != n or int(bits.shape[1]) != int(H):
            raise ValueError(f"postprocess_small_regions: {len(meta)} records and H = {H} for a stack of {tuple(bits.shape)}")
        if n == 0:
            return bits, []
        rec = (_lib.MaskMeta * n)()
        for i, m in enumerate(meta):
            C.memmove(C.byref(rec[i]), C.byref(m), C.sizeof(_lib.MaskMeta))
        out = torch.empty_like(bits)
        cnt = C.c_int(0)
        self._check(self.lib.saber_amg_postprocess_small_regions(self.h, _ptr(bits), n, int(H), int(W), rec, int(min_area), float(nms_thresh), _ptr(out),
                                                                 C.byref(cnt), _stream()))
        return out[:cnt.value], [rec[i] for i in range(cnt.value)]

    # ------------------------------------------------------------------ run-length output (csrc/rle.hip)
    def rle_encode(self, bits: torch.Tensor, W: int):
        """Upstream's uncompressed RLE of every mask of a bit-packed (n,H,W32) int32 device stack (include/saber_amd_kernels.h:
        saber_k_rle_count, saber_k_rle_encode): column-major runs, zeros first.  Returns device tensors (counts int32 (total,), offsets int64
        (n + 1,)): mask i owns counts[offsets[i]:offsets[i + 1]].  `offsets` is read back once to size `counts`: the call's one host wait
        (the encode's capacity check re-reads its last entry on the then idle stream)."""
        if not torch.cuda.is_available():
            raise RuntimeError("saber_amd.Engine.rle_encode needs a ROCm device; there is no CPU fallback")
        bits = self._check_packed("rle_encode", bits, W)
        n, H, W = int(bits.shape[0]), int(bits.shape[1]), int(W)
        if H * W >= 2 ** 31:
            raise ValueError(f"rle_encode: masks of 2^31 pixels or more are not supported, got {H} x {W}")
        offsets = torch.zeros((n + 1,), dtype=torch.int64, device=self.device)
        if n == 0 or H == 0:
            return torch.empty((0,), dtype=torch.int32, device=self.device), offsets
        ws = torch.empty((int(self.lib.saber_k_rle_workspace_bytes(n, H, W)),), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            if self.lib.saber_k_rle_count(_ptr(bits), n, H, W, _ptr(offsets), _ptr(ws), ws.numel(), _stream()) != 0:
                raise ValueError(f"saber_amd: {self.lib.saber_k_last_error().decode()}")
            total = int(offsets[n].item())                     # the host wait
            counts = torch.empty((total,), dtype=torch.int32, device=self.device)
            if self.lib.saber_k_rle_encode(_ptr(bits), n, H, W, _ptr(offsets), _ptr(counts), total, _ptr(ws), ws.numel(), _stream()) != 0:
                raise ValueError(f"saber_amd: {self.lib.saber_k_last_error().decode()}")
        return counts, offsets

    def rle_decode(self, counts: torch.Tensor, offsets: torch.Tensor, H: int, W: int) -> torch.Tensor:
        """The bit-packed (n,H,W32) int32 device stack of n masks given as uncompressed RLE (include/saber_amd_kernels.h: saber_k_rle_decode).
        counts: int32 / uint32 device tensor, offsets: int64 (n + 1,) device tensor, ascending, offsets[n] <= len(counts).  Runs are clamped at
        H W; padding bits are zero.  No host synchronisation."""
        if not torch.cuda.is_available():
            raise RuntimeError("saber_amd.Engine.rle_decode needs a ROCm device; there is no CPU fallback")
        for name, t, dtypes in (("counts", counts, (torch.int32, torch.uint32)), ("offsets", offsets, (torch.int64,))):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dtypes or t.dim() != 1:
                raise ValueError(f"rle_decode: {name} must be a 1-D device tensor of {' / '.join(str(d) for d in dtypes)}")
            if t.device != self.device:
                raise ValueError(f"rle_decode: {name} is on {t.device}, the engine on {self.device}")
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H * W >= 2 ** 31 or offsets.numel() < 1:
            raise ValueError(f"rle_decode: H and W of at least 1 with H W < 2^31 and n + 1 offsets are needed, got {H} x {W}, {offsets.numel()} offsets")
        counts, offsets = counts.contiguous(), offsets.contiguous()
        n = int(offsets.numel()) - 1
        bits = torch.empty((n, H, (W + 31) // 32), dtype=torch.int32, device=self.device)
        if n == 0:
            return bits
        if counts.numel() == 0:
            raise ValueError("rle_decode: every mask has at least one entry, got no counts")
        with torch.cuda.device(self.device):
            if self.lib.saber_k_rle_decode(_ptr(counts), _ptr(offsets), n, H, W, _ptr(bits), _stream()) != 0:
                raise ValueError(f"saber_amd: {self.lib.saber_k_last_error().decode()}")
        return bits

    def label_plane(self, bits: torch.Tensor, order: Sequence[int], H: int, W: int) -> torch.Tensor:
        plane = torch.empty((H, W), dtype=torch.uint16, device=self.device)
        n = len(order)
        arr = (C.c_int * max(n, 1))(*order)
        self._check(self.lib.saber_label_plane(self.h, _ptr(bits) if n else None, arr, n, H, W, _ptr(plane), _stream()))
        return plane

    def pair_intersections(self, bits: torch.Tensor, H: int, W: int) -> torch.Tensor:
        n = bits.shape[0]
        inter = torch.empty((n, n), dtype=torch.int32, device=self.device)
        self._check(self.lib.saber_mask_pair_intersections(self.h, _ptr(bits) if n else None, n, H, W, _ptr(inter) if n else None, _stream()))
        return inter

    # ------------------------------------------------------------------ sliding-window masks (csrc/windows.hip)
    def _check_window_src(self, who: str, src):
        if not torch.cuda.is_available():
            raise RuntimeError(f"saber_amd.Engine.{who} needs a ROCm device; there is no CPU fallback")
        if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype not in (torch.int32, torch.uint32) or src.dim() != 1:
            raise ValueError(f"{who}: src must be a 1-D int32 device tensor of packed window rows")
        if src.device != self.device:
            raise ValueError(f"{who}: src is on {src.device}, the engine on {self.device}")
        return src.contiguous()

    def place_window_masks(self, src: torch.Tensor, table, H: int, W: int) -> torch.Tensor:
        """Window-sized bit-packed masks in full-frame rows (include/saber_amd.h: saber_place_window_masks): the generator's layout of what
        saber2D.rasterize_masks builds as bool arrays.  src: 1-D int32 device tensor, table: the n records (src_word, y0, x0, h, w) - a
        sequence of tuples or a _lib.window_table.  Returns (n, H, ceil(W/32)) int32, zero outside each window.  Every record is checked
        on the host (ValueError naming it) before anything is launched.  One launch, no host synchronisation."""
        src = self._check_window_src("place_window_masks", src)
        n = len(table)
        tab = _lib.window_table(table)
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"place_window_masks: H and W must be at least 1, got {H} x {W}")
        out = torch.empty((n, H, (W + 31) // 32), dtype=torch.int32, device=self.device)
        self._check(self.lib.saber_place_window_masks(self.h, _ptr(src), src.numel(), tab, n, H, W, _ptr(out), _stream()))
        return out

    def window_label_stack(self, src: torch.Tensor, table, H: int, W: int, first: int = 0, count: Optional[int] = None,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Planes first .. first + count - 1 of the filters.masks.masks_to_array stack of the n window masks of `table`, written straight from
        the window rows (include/saber_amd.h: saber_window_label_stack): plane i holds first + i + 1 where mask first + i covers the pixel.
        The element type follows the TOTAL number of masks n, as masks_to_array's does: uint8 below 256, then 2 bytes below 65536, then 4 -
        returned as uint8 / int16 / int32 (torch has no unsigned 16- / 32-bit arithmetic; view the download as np.uint16 / np.uint32).
        out: an optional contiguous (count,H,W) device tensor of that type to write into.  One launch, no host synchronisation."""
        src = self._check_window_src("window_label_stack", src)
        n = len(table)
        first = int(first)
        count = n - first if count is None else int(count)
        H, W = int(H), int(W)
        if first < 0 or count < 0 or first + count > n:
            raise ValueError(f"window_label_stack: planes {first} .. {first + count} of {n} masks")
        if H < 1 or W < 1:
            raise ValueError(f"window_label_stack: H and W must be at least 1, got {H} x {W}")
        dtype = window_stack_dtype(n)
        if out is None:
            out = torch.empty((count, H, W), dtype=dtype, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != dtype or tuple(out.shape) != (count, H, W)
              or not out.is_contiguous()):
            raise ValueError(f"window_label_stack: out must be a contiguous ({count},{H},{W}) {dtype} tensor on {self.device}")
        self._check(self.lib.saber_window_label_stack(self.h, _ptr(src), src.numel(), _lib.window_table(table), n, first, count, H, W,
                                                      out.element_size(), _ptr(out), _stream()))
        return out

    def unpack_masks(self, bits: torch.Tensor, W: int) -> np.ndarray:
        """(n,H,W32) int32 device stack -> (n,H,W) bool numpy, unpacked on the device (unpack_bits below)"""
        return unpack_bits(self._check_packed("unpack_masks", bits, W), int(W))

    def separate_masks(self, planes: torch.Tensor, min_mask_area: int = 100):
        """utils.separate_masks on the device.  planes: (Z,H,W) uint16 / int16 device tensor of per-slice label planes.
        Returns ((Z,H,W) int32 device tensor holding the uint32 labels, number of labels)."""
        assert planes.is_cuda and planes.dim() == 3 and planes.is_contiguous() and planes.dtype in (torch.uint16, torch.int16)
        Z, H, W = planes.shape
        out = torch.empty((Z, H, W), dtype=torch.int32, device=planes.device)
        n = C.c_int(0)
        self._check(self.lib.saber_separate_masks(self.h, _ptr(planes), Z, H, W, int(min_mask_area), _ptr(out), C.byref(n), _stream()))
        return out, n.value

    # ------------------------------------------------------------------ the stitch over z-chunks (csrc/cc3d.hip, segmenters/stitch.py)
    def _check_chunk(self, who: str, lab: torch.Tensor, sizes: torch.Tensor):
        for name, t in (("lab", lab), ("sizes", sizes)):
            if (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.int32 or t.dim() != 3 or not t.is_contiguous()
                    or t.numel() == 0):
                raise ValueError(f"{who}: {name} must be a non-empty contiguous (Z,H,W) int32 tensor on {self.device}")
        if lab.shape != sizes.shape:
            raise ValueError(f"{who}: lab {tuple(lab.shape)} and sizes {tuple(sizes.shape)} differ in shape")
        return lab.shape

    @staticmethod
    def _root_list(who: str, what: str, roots) -> np.ndarray:
        a = np.asarray(roots)
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise ValueError(f"{who}: {what} must hold voxel indices of the chunk")
        return np.ascontiguousarray(a.reshape(-1), dtype=np.uint32)

    def cc_chunk_label(self, planes: torch.Tensor):
        """The labelling of separate_masks on one z-chunk.  planes: (Z,H,W) uint16 / int16 device tensor.  Returns (lab, sizes), both
        (Z,H,W) int32 holding uint32: lab[v] = the chunk-local root of v (its component's first voxel in scan order; -1 = background),
        sizes[root] = the component's voxels inside the chunk.  No host synchronisation."""
        if (not isinstance(planes, torch.Tensor) or planes.device != self.device or planes.dim() != 3 or not planes.is_contiguous()
                or planes.dtype not in (torch.uint16, torch.int16) or planes.numel() == 0):
            raise ValueError(f"cc_chunk_label: planes must be a non-empty contiguous (Z,H,W) uint16 / int16 tensor on {self.device}")
        Z, H, W = planes.shape
        lab = torch.empty((Z, H, W), dtype=torch.int32, device=self.device)
        sizes = torch.empty((Z, H, W), dtype=torch.int32, device=self.device)
        self._check(self.lib.saber_cc_chunk_label(self.h, _ptr(planes), Z, H, W, _ptr(lab), _ptr(sizes), _stream()))
        return lab, sizes

    def cc_seam_pairs(self, a_roots: torch.Tensor, b_roots: torch.Tensor, a_offset: int = 0, b_offset: int = 0,
                      capacity: Optional[int] = None) -> np.ndarray:
        """The roots that touch across a seam.  a_roots: a chunk's last (H,W) plane of `lab`, b_roots: the next chunk's first one (int32
        device tensors, -1 = background); the offsets (z0 * H * W of either chunk) turn chunk-local roots into global voxel indices.
        Returns the (k,2) int64 array of unique rows (root in a, root in b), sorted.  capacity: rows of the device buffer of the first
        attempt (default H * W); a seam with more is run once more with the count the kernel reported."""
        for name, t in (("a_roots", a_roots), ("b_roots", b_roots)):
            if (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.int32 or t.dim() != 2 or not t.is_contiguous()
                    or t.numel() == 0):
                raise ValueError(f"cc_seam_pairs: {name} must be a non-empty contiguous (H,W) int32 tensor on {self.device}")
        if a_roots.shape != b_roots.shape:
            raise ValueError(f"cc_seam_pairs: the planes differ in shape, {tuple(a_roots.shape)} and {tuple(b_roots.shape)}")
        H, W = a_roots.shape
        cap = H * W if capacity is None else int(capacity)
        if cap < 0 or not 0 <= int(a_offset) <= 0x7FFFFFFF or not 0 <= int(b_offset) <= 0x7FFFFFFF:
            raise ValueError("cc_seam_pairs: capacity and offsets must not be negative (offsets below 2^31)")
        n = C.c_int(0)
        for _ in range(2):
            buf = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=self.device)
            st = self.lib.saber_cc_seam_pairs(self.h, _ptr(a_roots), _ptr(b_roots), H, W, int(a_offset), int(b_offset), _ptr(buf), cap, C.byref(n),
                                              _stream())
            if st != _lib.SABER_ERR_CAPACITY:
                break
            cap = n.value                      # the kernel counted every pair: room for all of them now
        self._check(st)
        rows = buf[:n.value].cpu().numpy().view(np.uint32).astype(np.int64)
        return np.unique(rows, axis=0) if rows.size else rows.reshape(0, 2)

    def cc_chunk_roots(self, lab: torch.Tensor, sizes: torch.Tensor, min_voxels: int, exclude=()) -> np.ndarray:
        """The chunk-local roots with at least max(min_voxels, 1) voxels that are not in `exclude` (the roots that face a seam), ascending
        (int64).  sizes[root] is cleared for the excluded and the smaller roots."""
        Z, H, W = self._check_chunk("cc_chunk_roots", lab, sizes)
        ex = self._root_list("cc_chunk_roots", "exclude", exclude)
        if not 0 <= int(min_voxels) <= 0xFFFFFFFF:
            raise ValueError(f"cc_chunk_roots: min_voxels {min_voxels} out of range")
        n = C.c_int(0)
        cap = 4096
        for _ in range(2):
            out = np.empty(cap, dtype=np.uint32)
            st = self.lib.saber_cc_chunk_roots(self.h, _ptr(lab), _ptr(sizes), Z, H, W, int(min_voxels), ex.ctypes.data_as(C.c_void_p) if ex.size else None,
                                               int(ex.size), out.ctypes.data_as(C.c_void_p), cap, C.byref(n), _stream())
            if st != _lib.SABER_ERR_CAPACITY or n.value <= cap:
                break
            cap = n.value                      # the clearing is idempotent: the call may be repeated
        self._check(st)
        return out[:n.value].astype(np.int64)

    def cc_chunk_finish(self, lab: torch.Tensor, sizes: torch.Tensor, roots, ids) -> torch.Tensor:
        """Gives the listed chunk-local roots their ids and relabels the chunk: returns `sizes`, now the (Z,H,W) int32 tensor holding the
        chunk's uint32 labels (every root not listed, and the background, is 0).  To be called after cc_chunk_roots."""
        Z, H, W = self._check_chunk("cc_chunk_finish", lab, sizes)
        r = self._root_list("cc_chunk_finish", "roots", roots)
        i = self._root_list("cc_chunk_finish", "ids", ids)
        if r.size != i.size:
            raise ValueError(f"cc_chunk_finish: {r.size} roots and {i.size} ids")
        self._check(self.lib.saber_cc_chunk_finish(self.h, _ptr(lab), _ptr(sizes), Z, H, W, r.ctypes.data_as(C.c_void_p) if r.size else None,
                                                   i.ctypes.data_as(C.c_void_p) if i.size else None, int(r.size), _stream()))
        return sizes

    def smooth_labels(self, labels: torch.Tensor, scale: float = 0.075):
        """filters.masks.fast_3d_gaussian_smoothing on the device.  labels: (Z,H,W) device tensor of uint8 / (u)int16 / (u)int32 label
        values (non-negative).  Returns ((Z,H,W) uint8 device tensor, number of labels found)."""
        assert labels.is_cuda and labels.dim() == 3 and labels.is_contiguous()
        if labels.dtype not in (torch.uint8, torch.int16, torch.uint16, torch.int32, torch.uint32):
            raise ValueError(f"smooth_labels: unsupported dtype {labels.dtype}")
        Z, H, W = labels.shape
        out = torch.empty((Z, H, W), dtype=torch.uint8, device=labels.device)
        n = C.c_int(0)
        self._check(self.lib.saber_smooth_labels(self.h, _ptr(labels), labels.element_size(), Z, H, W, float(scale), _ptr(out), C.byref(n), _stream()))
        return out, n.value

    # ------------------------------------------------------------------ smoothing over z-chunks (csrc/smooth3d.hip, segmenters/smooth.py)
    _LABEL_DTYPES = (torch.uint8, torch.int16, torch.uint16, torch.int32, torch.uint32)

    def _check_label_planes(self, who: str, name: str, t, hw=None, allow_empty: bool = False):
        if (not isinstance(t, torch.Tensor) or t.device != self.device or t.dim() != 3 or not t.is_contiguous()
                or t.dtype not in self._LABEL_DTYPES or (t.shape[0] == 0 and not allow_empty) or t.shape[1] == 0 or t.shape[2] == 0):
            raise ValueError(f"{who}: {name} must be a {'' if allow_empty else 'non-empty '}contiguous (Z,H,W) uint8 / (u)int16 / (u)int32 tensor on {self.device}")
        if hw is not None and tuple(t.shape[1:]) != tuple(hw):
            raise ValueError(f"{who}: {name} has planes of {tuple(t.shape[1:])}, the chunk's are {tuple(hw)}")

    def smooth_radius(self, count: int, scale: float) -> int:
        """The tap radius smooth_labels / smooth_labels_chunk use for a label of `count` voxels (the library's own arithmetic)."""
        r = C.c_int(0)
        if self.lib.saber_smooth_radius(int(count), float(scale), C.byref(r)) != _lib.SABER_OK:
            raise ValueError(f"smooth_radius: count {count} must not be negative and scale {scale} must be positive")
        return r.value

    def label_max(self, labels: torch.Tensor) -> int:
        """The largest label value of a (Z,H,W) uint8 / (u)int16 / (u)int32 device tensor (elements read as unsigned)."""
        self._check_label_planes("label_max", "labels", labels)
        m = C.c_uint32(0)
        self._check(self.lib.saber_label_max(self.h, _ptr(labels), labels.element_size(), labels.numel(), C.byref(m), _stream()))
        return m.value

    def label_counts(self, labels: torch.Tensor, n: int) -> torch.Tensor:
        """counts[v] = voxels of label value v for 0 < v < n, counts[0] = 0 (the background is not counted): an (n,) int64 device tensor.
        Every value of `labels` must be below n."""
        self._check_label_planes("label_counts", "labels", labels)
        if not 1 <= int(n) <= (1 << 22) + 1:
            raise ValueError(f"label_counts: a table of {n} entries (label values lie in [0, 2^22])")
        out = torch.empty((int(n),), dtype=torch.int64, device=self.device)
        Z, H, W = labels.shape
        self._check(self.lib.saber_label_counts(self.h, _ptr(labels), labels.element_size(), Z, H, W, int(n), _ptr(out), _stream()))
        return out

    def smooth_labels_chunk(self, own: torch.Tensor, lo: Optional[torch.Tensor], hi: Optional[torch.Tensor], ids, counts, scale: float,
                            lo_end: bool, hi_end: bool):
        """smooth_labels on one z-chunk of a larger volume.  own: the chunk's (Zc,H,W) label planes; lo / hi: the planes right below / above
        it (None or 0 planes: none), same dtype and H x W; ids, counts: the label values of the whole volume, ascending, and their voxel
        counts there; lo_end / hi_end: the halo ends where the volume ends.  A halo must hold max(smooth_radius(count, scale)) planes unless
        it is the volume's end.  Returns ((Zc,H,W) uint8 device tensor - bit for bit smooth_labels of the whole volume on these planes -
        and the number of labels convolved)."""
        who = "smooth_labels_chunk"
        self._check_label_planes(who, "own", own)
        Zc, H, W = own.shape
        halos = []
        for name, t in (("lo", lo), ("hi", hi)):
            if t is not None:
                self._check_label_planes(who, name, t, hw=(H, W), allow_empty=True)
                if t.dtype != own.dtype:
                    raise ValueError(f"{who}: {name} is {t.dtype}, own is {own.dtype}")
            halos.append(t if t is not None and t.shape[0] else None)
        lo, hi = halos
        ids = np.ascontiguousarray(np.asarray(ids).reshape(-1))
        counts = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.int64)
        if ids.size != counts.size:
            raise ValueError(f"{who}: {ids.size} ids and {counts.size} counts")
        if ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF):
            raise ValueError(f"{who}: ids must be label values")
        ids = ids.astype(np.uint32)
        out = torch.empty((Zc, H, W), dtype=torch.uint8, device=self.device)
        n = C.c_int(0)
        self._check(self.lib.saber_smooth_labels_chunk(
            self.h, _ptr(lo) if lo is not None else None, lo.shape[0] if lo is not None else 0, _ptr(own), Zc,
            _ptr(hi) if hi is not None else None, hi.shape[0] if hi is not None else 0, int(bool(lo_end)), int(bool(hi_end)), own.element_size(),
            H, W, ids.ctypes.data_as(C.c_void_p) if ids.size else None, counts.ctypes.data_as(C.c_void_p) if ids.size else None, int(ids.size),
            float(scale), _ptr(out), C.byref(n), _stream()))
        return out, n.value

    def gaussian_smoothing_3d(self, mask: torch.Tensor, sigma: float) -> torch.Tensor:
        """filters.gaussian.gaussian_smoothing_3d on the device.  mask: (Z,H,W) bool / uint8 0-1 device tensor -> float32 field."""
        assert mask.is_cuda and mask.dim() == 3 and mask.is_contiguous() and mask.dtype in (torch.bool, torch.uint8)
        Z, H, W = mask.shape
        out = torch.empty((Z, H, W), dtype=torch.float32, device=mask.device)
        self._check(self.lib.saber_gaussian_smoothing_3d(self.h, _ptr(mask), Z, H, W, float(sigma), _ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ membrane refinement (csrc/morph3d.hip)
    def morph_ball_3d(self, mask: torch.Tensor, radius: int, op: int) -> torch.Tensor:
        """Binary dilation (op 0), erosion (1) or opening (2) by the ball of `radius` 1..16, zero border.  mask: (Z,H,W) bool / uint8
        device tensor -> uint8 0/1."""
        assert mask.is_cuda and mask.dim() == 3 and mask.is_contiguous() and mask.dtype in (torch.bool, torch.uint8)
        Z, H, W = mask.shape
        out = torch.empty((Z, H, W), dtype=torch.uint8, device=mask.device)
        self._check(self.lib.saber_morph_ball_3d(self.h, _ptr(mask), Z, H, W, int(radius), int(op), _ptr(out), _stream()))
        return out

    def components6_3d(self, mask: torch.Tensor, mode: int, min_size: int = 0):
        """6-connected components of a (Z,H,W) bool / uint8 device tensor.  mode 0: zero the components below min_size; mode 1: keep
        the largest (first in raster order on ties).  Returns (uint8 tensor, components kept (mode 0) / found (mode 1))."""
        assert mask.is_cuda and mask.dim() == 3 and mask.is_contiguous() and mask.dtype in (torch.bool, torch.uint8)
        Z, H, W = mask.shape
        out = torch.empty((Z, H, W), dtype=torch.uint8, device=mask.device)
        n = C.c_int(0)
        self._check(self.lib.saber_components6_3d(self.h, _ptr(mask), Z, H, W, int(mode), int(min_size), _ptr(out), C.byref(n), _stream()))
        return out, n.value

    def refine_membranes(self, org: torch.Tensor, mem: torch.Tensor, params: "_lib.RefineParams"):
        """OrganelleMembraneFilter.run on the device.  org: (Z,H,W) uint8 / (u)int16 / (u)int32 labels, mem: (Z,H,W) bool / uint8.
        Returns (organelle label map, membrane label map, surviving pairs); the maps have org's dtype, organelle v comes out as v + 1."""
        assert org.is_cuda and org.dim() == 3 and org.is_contiguous() and mem.is_cuda and mem.is_contiguous() and mem.shape == org.shape
        if org.dtype not in (torch.uint8, torch.int16, torch.uint16, torch.int32, torch.uint32):
            raise ValueError(f"refine_membranes: unsupported label dtype {org.dtype}")
        if mem.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"refine_membranes: the membrane volume must be bool or uint8, got {mem.dtype}")
        Z, H, W = org.shape
        org_out, mem_out = torch.empty_like(org), torch.empty_like(org)
        n_in, n_pairs = C.c_int(0), C.c_int(0)
        self._check(self.lib.saber_refine_membranes(self.h, _ptr(org), org.element_size(), _ptr(mem), Z, H, W, C.byref(params), _ptr(org_out),
                                                    _ptr(mem_out), C.byref(n_in), C.byref(n_pairs), _stream()))
        self.refine_labels_in = n_in.value
        return org_out, mem_out, n_pairs.value

    def refine_membranes_instances(self, first: int, count: int, shape, dtype: torch.dtype):
        """Pairs [first, first + count) of the last refine_membranes call as two (count,Z,H,W) device stacks of `dtype`."""
        org = torch.empty((count,) + tuple(shape), dtype=dtype, device=self.device)
        mem = torch.empty_like(org)
        self._check(self.lib.saber_refine_membranes_instances(self.h, int(first), int(count), org.element_size(), _ptr(org), _ptr(mem), _stream()))
        return org, mem

    # ------------------------------------------------------------------ organelle statistics (csrc/labelstats.hip)
    def label_statistics(self, labels: torch.Tensor, capacity: int = 1024, per_piece_atomics: bool = False):
        """Per-label moments of a (Z,H,W) uint8 / (u)int16 / (u)int32 device tensor (include/saber_amd.h: saber_label_statistics).
        Returns device tensors with one row per label > 0, ascending: (labels int32[K], moments int64[K,16], stats float64[K,8]); the
        unsigned values of the C-ABI fit the signed types.  `capacity` is a first guess: the call is repeated once with the K it reports.
        per_piece_atomics selects the unreduced baseline form of the moments kernel (same results, for measurements)."""
        assert labels.is_cuda and labels.dim() == 3 and labels.is_contiguous()
        if labels.dtype not in (torch.uint8, torch.int16, torch.uint16, torch.int32, torch.uint32):
            raise ValueError(f"label_statistics: unsupported label dtype {labels.dtype}")
        Z, H, W = labels.shape
        signed = int(labels.dtype in (torch.int16, torch.int32))
        n = C.c_int(0)
        while True:
            lab = torch.empty((capacity,), dtype=torch.int32, device=labels.device)
            mom = torch.empty((capacity, 16), dtype=torch.int64, device=labels.device)
            stats = torch.empty((capacity, 8), dtype=torch.float64, device=labels.device)
            st = self.lib.saber_label_statistics(self.h, _ptr(labels), labels.element_size(), signed, Z, H, W, int(capacity), int(bool(per_piece_atomics)),
                                                 _ptr(lab), _ptr(mom), _ptr(stats), C.byref(n), _stream())
            if st == _lib.SABER_ERR_CAPACITY and n.value > capacity:
                capacity = n.value
                continue
            self._check(st)
            return lab[:n.value], mom[:n.value], stats[:n.value]

    # ------------------------------------------------------------------ consensus mask resolution (csrc/consensus2d.hip)
    # one row of the C-ABI's saber_consensus_row table as the host reads it
    CONSENSUS_ROW = np.dtype([("area", np.int32), ("x_min", np.int32), ("y_min", np.int32), ("x_max", np.int32), ("y_max", np.int32),
                              ("reserved", np.int32), ("avg_sum", np.float64)])

    def consensus_components(self, masks_u8: torch.Tensor, select: Sequence[int], conf, capacity: Optional[int] = None):
        """4-connected components of the union of the selected masks and their consensus table (include/saber_amd.h:
        saber_consensus_components).  masks_u8: (n,H,W) uint8 device tensor, non-zero = set; select: k row indices in list order; conf:
        their k confidences (cast to float32).  Returns (labels, table): labels is the (H,W) int32 device tensor, 0 = background and
        1..K in scipy.ndimage.label's order; table maps "area", "x_min", "y_min", "x_max", "y_max" (int64 numpy arrays) and "score"
        (float64: the component's mean overlap-averaged confidence) to K entries, ascending label.  `capacity` is a first guess of K
        (default: ceil(H W / 2) rows, which always suffice, at most 65536); the call is repeated once with the K it reports.
        Two host synchronisations: the end of the device work, and the download of the table."""
        if not isinstance(masks_u8, torch.Tensor) or not masks_u8.is_cuda:
            raise ValueError("consensus_components: the mask stack must be a device tensor")
        if masks_u8.dtype != torch.uint8 or masks_u8.dim() != 3:
            raise ValueError(f"consensus_components: the mask stack must be (n,H,W) uint8, got {tuple(masks_u8.shape)} {masks_u8.dtype}")
        if masks_u8.device != self.device:
            raise ValueError(f"consensus_components: the mask stack is on {masks_u8.device}, the engine on {self.device}")
        masks_u8 = masks_u8.contiguous()
        sel = np.ascontiguousarray(np.asarray(select, dtype=np.int64).reshape(-1))
        cf = np.ascontiguousarray(np.asarray(conf).reshape(-1).astype(np.float32))
        n, H, W = masks_u8.shape
        if sel.size != cf.size:
            raise ValueError(f"consensus_components: {sel.size} selected masks, {cf.size} confidences")
        if sel.size == 0 or sel.size > n or sel.min() < 0 or sel.max() >= n or n == 0 or H == 0 or W == 0 or H * W >= 2 ** 31 - 1:
            raise ValueError(f"consensus_components: a selection of 1..n rows of a non-empty (n,H,W) stack with H W < 2^31 is needed, got "
                             f"{sel.size} of {tuple(masks_u8.shape)}")
        return self._consensus_run(self.lib.saber_consensus_components, masks_u8, n, H, W, sel, cf, capacity)

    def _consensus_run(self, entry, stack: torch.Tensor, n: int, H: int, W: int, sel: np.ndarray, cf: np.ndarray, capacity: Optional[int]):
        """the capacity protocol and the table download both consensus entries share (stack: the uint8 or the bit-packed tensor)"""
        sel = sel.astype(np.int32)
        if capacity is None:
            capacity = min((H * W + 1) // 2, 65536)
        labels = torch.empty((H, W), dtype=torch.int32, device=stack.device)
        k = C.c_int(0)
        with torch.cuda.device(self.device):
            while True:
                table = torch.empty((max(int(capacity), 1), self.CONSENSUS_ROW.itemsize), dtype=torch.uint8, device=stack.device)
                st = entry(self.h, _ptr(stack), n, H, W, sel.ctypes.data_as(C.POINTER(C.c_int)), cf.ctypes.data_as(C.POINTER(C.c_float)),
                           int(sel.size), int(capacity), _ptr(labels), _ptr(table), C.byref(k), _stream())
                if st == _lib.SABER_ERR_CAPACITY and k.value > capacity:
                    capacity = k.value
                    continue
                self._check(st)
                break
        rows = table[:k.value].cpu().numpy().view(self.CONSENSUS_ROW).reshape(-1)
        out = {name: rows[name].astype(np.int64) for name in ("area", "x_min", "y_min", "x_max", "y_max")}
        out["score"] = rows["avg_sum"] / np.maximum(rows["area"], 1).astype(np.float64)
        return labels, out

    def consensus_components_bits(self, bits: torch.Tensor, W: int, select: Sequence[int], conf, capacity: Optional[int] = None):
        """consensus_components on rows of the mask generator's bit-packed stack (include/saber_amd.h: saber_consensus_components_bits).
        bits: (n,H,W32) int32 / uint32 device tensor as amg_generate returns it (bit b of word w = pixel 32w+b), W: the image width;
        select, conf, capacity and the returned (labels, table) as in consensus_components.  No uint8 stack is made."""
        if not isinstance(bits, torch.Tensor) or not bits.is_cuda:
            raise ValueError("consensus_components_bits: the mask stack must be a device tensor")
        if bits.dtype not in (torch.int32, torch.uint32) or bits.dim() != 3 or bits.shape[2] != (int(W) + 31) // 32:
            raise ValueError(f"consensus_components_bits: the mask stack must be (n,H,ceil(W/32)) int32 for W = {W}, got {tuple(bits.shape)} {bits.dtype}")
        if bits.device != self.device:
            raise ValueError(f"consensus_components_bits: the mask stack is on {bits.device}, the engine on {self.device}")
        bits = bits.contiguous()
        sel = np.ascontiguousarray(np.asarray(select, dtype=np.int64).reshape(-1))
        cf = np.ascontiguousarray(np.asarray(conf).reshape(-1).astype(np.float32))
        n, H, W = int(bits.shape[0]), int(bits.shape[1]), int(W)
        if sel.size != cf.size:
            raise ValueError(f"consensus_components_bits: {sel.size} selected masks, {cf.size} confidences")
        if sel.size == 0 or sel.size > n or sel.min() < 0 or sel.max() >= n or n == 0 or H == 0 or W == 0 or H * W >= 2 ** 31 - 1:
            raise ValueError(f"consensus_components_bits: a selection of 1..n rows of a non-empty (n,H,W32) stack with H W < 2^31 is needed, got "
                             f"{sel.size} of {tuple(bits.shape)}")
        return self._consensus_run(self.lib.saber_consensus_components_bits, bits, n, H, W, sel, cf, capacity)

    def relabel_plane(self, labels: torch.Tensor, lut) -> torch.Tensor:
        """plane[p] = lut[labels[p]] (include/saber_amd.h: saber_relabel_plane).  labels: (H,W) int32 device tensor (a consensus call's
        label plane), lut: K + 1 uint16 values, lut[0] = 0, as a numpy array (uploaded here) or a device tensor of int16 / uint16.
        Returns the (H,W) uint16 device plane; no host synchronisation."""
        if not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dtype != torch.int32 or labels.dim() != 2:
            raise ValueError("relabel_plane: labels must be an (H,W) int32 device tensor")
        if labels.device != self.device:
            raise ValueError(f"relabel_plane: the labels are on {labels.device}, the engine on {self.device}")
        if not isinstance(lut, torch.Tensor):
            lut = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.uint16).reshape(-1).view(np.int16)).to(self.device)
        if lut.dtype not in (torch.int16, torch.uint16) or lut.dim() != 1 or lut.numel() < 1 or lut.device != self.device:
            raise ValueError("relabel_plane: lut must hold at least one uint16 value on the engine's device")
        labels, lut = labels.contiguous(), lut.contiguous()
        H, W = labels.shape
        plane = torch.empty((H, W), dtype=torch.uint16, device=self.device)
        if H * W:
            self._check(self.lib.saber_relabel_plane(self.h, _ptr(labels), H, W, _ptr(lut), int(lut.numel()), _ptr(plane), _stream()))
        return plane

    def set_precision(self, precision: str):
        """Switch between the handle's 16-bit production arithmetic ("bf16" or "fp16": whichever its weights were converted to) and the
        fp32 exact mode (only on a handle created with precision="exact", which keeps the fp32 weight copies)."""
        if precision not in ("bf16", "fp16", "exact"):
            raise ValueError(f"precision must be 'bf16', 'fp16' or 'exact', got '{precision}'")
        self._check(self.lib.saber_engine_set_precision(self.h, {"bf16": 0, "exact": 1, "fp16": 2}[precision]))
        self.precision = precision

    def set_encoder_stream(self, stream_ptr):
        """The mask generator's encoder passes on another HIP stream (include/saber_amd.h: saber_engine_set_encoder_stream); None = default."""
        self._check(self.lib.saber_engine_set_encoder_stream(self.h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def set_device_amg(self, enable: bool):
        """Filters / NMS / compaction of the mask generator on the device (default) or on the host (include/saber_amd.h: saber_engine_set_device_amg)."""
        self._check(self.lib.saber_engine_set_device_amg(self.h, int(bool(enable))))

    def set_iou_pruning(self, enable: bool):
        """IoU pruning of the AMG m2m pass (include/saber_amd.h: saber_engine_set_iou_pruning); on by default, results identical."""
        self._check(self.lib.saber_engine_set_iou_pruning(self.h, int(bool(enable))))

    def set_multipoint(self, enable: bool):
        """Prompts of 2..9 points (decode_prompts) on the handle's 16-bit kernels: the 16-token route (include/saber_amd.h:
        saber_engine_set_multipoint); off by default, where such prompts need the exact precision mode.  ValueError with max_prompts < 2."""
        self._check(self.lib.saber_engine_set_multipoint(self.h, int(bool(enable))))
        self.multipoint = bool(enable)

    def last_pruning(self):
        """(m2m candidates skipped, m2m candidates) of the last amg_generate call"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.saber_amg_last_pruning(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_graphs(self, enable: bool):
        """hipGraph replay of the AMG launch sequences (include/saber_amd.h: saber_engine_set_graphs)."""
        self._check(self.lib.saber_engine_set_graphs(self.h, int(bool(enable))))

    def graph_stats(self):
        """(sequences captured, sequences replayed) on this handle."""
        import ctypes as C
        c, r = C.c_int(0), C.c_int(0)
        self._check(self.lib.saber_engine_graph_stats(self.h, C.byref(c), C.byref(r)))
        return c.value, r.value

    def profile_begin(self):
        self._check(self.lib.saber_profile_begin(self.h))

    def profile_end(self) -> dict:
        n = len(_lib.PROFILE_CLASSES)
        arr = (_lib.ProfileClass * n)()
        self._check(self.lib.saber_profile_end(self.h, arr, n))
        return {name: {"launches": int(arr[i].launches), "ms": float(arr[i].ms), "flops": float(arr[i].flops), "bytes": float(arr[i].bytes)}
                for i, name in enumerate(_lib.PROFILE_CLASSES)}

    def encoder_flops(self) -> float:
        return float(self.lib.saber_encoder_flops(self.h))


def _check_cleanup_areas(who: str, max_hole_area, max_sprinkle_area):
    for name, v in (("max_hole_area", max_hole_area), ("max_sprinkle_area", max_sprinkle_area)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 65535:
            raise ValueError(f"{who}: {name} must be an integer from 0 to 65535, got {v!r}")


def lowres_cleanup_env_defaults():
    """(max_hole_area, max_sprinkle_area) from SABER_AMD_MAX_HOLE_AREA / SABER_AMD_MAX_SPRINKLE_AREA; unset or empty = 0."""
    out = []
    for var in ("SABER_AMD_MAX_HOLE_AREA", "SABER_AMD_MAX_SPRINKLE_AREA"):
        txt = os.environ.get(var, "").strip()
        try:
            v = int(txt) if txt else 0
        except ValueError:
            raise ValueError(f"{var} must be an integer from 0 to 65535, got {txt!r}") from None
        _check_cleanup_areas(var, v, 0)
        out.append(v)
    return tuple(out)


def window_stack_dtype(n: int) -> torch.dtype:
    """the element type of Engine.window_label_stack for n masks in all: filters.masks.masks_to_array's rule (uint8 below 256 masks, uint16
    below 65536, uint32 beyond) in the torch types that carry those bytes"""
    return torch.uint8 if n < 256 else (torch.int16 if n < 65536 else torch.int32)


def unpack_bits(bits: torch.Tensor, W: int) -> np.ndarray:
    """(n,H,W32) int32 device tensor -> (n,H,W) bool numpy (bit b of word w = pixel 32w+b).  Unpacked on the device
    (saber_k_unpack_masks) and copied through a pinned buffer; the caller owns the returned array."""
    n, H = bits.shape[:2]
    if n == 0:
        return np.zeros((0, H, W), dtype=bool)
    assert bits.is_cuda and bits.is_contiguous() and bits.shape[2] == (W + 31) // 32
    lib = _lib.load()
    out = np.empty((n, H, W), dtype=np.uint8)
    step = max(1, (64 << 20) // (H * W))                      # masks per pass: 64 MiB of device + pinned staging
    dev = torch.empty((min(step, n), H, W), dtype=torch.uint8, device=bits.device)
    pin = torch.empty((min(step, n), H, W), dtype=torch.uint8, pin_memory=True)
    for i0 in range(0, n, step):
        k = min(step, n - i0)
        if lib.saber_k_unpack_masks(_ptr(bits[i0:i0 + k]), k, H, W, _ptr(dev), _stream()) != 0:
            raise _lib.SaberAmdError(lib.saber_k_last_error().decode())
        pin[:k].copy_(dev[:k], non_blocking=True)
        torch.cuda.current_stream(bits.device).synchronize()
        out[i0:i0 + k] = pin[:k].numpy()
    return out.view(np.bool_)


def make_amg_params(amg: Optional[dict] = None) -> "_lib.AmgParams":
    """cfgAMG dict (saber/adapters/sam2/amg.py:7-17) -> C struct, with the upstream defaults SABER does not pass."""
    a = dict(npoints=32, points_per_batch=64, pred_iou_thresh=0.7, stability_score_thresh=0.92, stability_score_offset=0.7,
             crop_n_layers=2, box_nms_thresh=0.7, crop_n_points_downscale_factor=2, use_m2m=True, multimask_output=True)
    a["crop_nms_thresh"] = 0.7          # upstream default; not a cfgAMG field (bench.py's tail mode and tests may override it)
    a.update({k: v for k, v in (amg or {}).items() if k in a})
    return _lib.AmgParams(points_per_side=a["npoints"], points_per_batch=a["points_per_batch"], pred_iou_thresh=a["pred_iou_thresh"],
                          stability_score_thresh=a["stability_score_thresh"], stability_score_offset=a["stability_score_offset"],
                          mask_threshold=0.0, box_nms_thresh=a["box_nms_thresh"], crop_n_layers=a["crop_n_layers"], crop_nms_thresh=a["crop_nms_thresh"],
                          crop_overlap_ratio=512 / 1500, crop_n_points_downscale_factor=a["crop_n_points_downscale_factor"],
                          use_m2m=int(a["use_m2m"]), multimask_output=int(a["multimask_output"]))
