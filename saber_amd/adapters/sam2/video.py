"""SAM2 video (memory) propagation on the MI355X engine: the host side of SURVEY.md 8f-1.

What `saber segment tomograms` runs after the seed slab (reference: saber/segmenters/tomo.py:81-139 -> SAM2Adapter.segment_volume,
saber/adapters/sam2/predictor.py:232-348, which drives the third-party video predictor: add_new_mask, propagate_in_video forwards
and backwards).  This module is the Python host of that loop; every arithmetic step is a HIP kernel behind the C-ABI:

    per frame        Hiera encoder + FPN neck                      saber_encode (engine.hip: the AMG path's kernels)
    memory attention 4 x [RoPE self-attention, RoPE cross-attention to the memory bank, MLP]
                     projections / scores / values / MLP           saber_k_gemm_ld (bf16 MFMA GEMM)
                     LayerNorm, RoPE, row softmax                  saber_k_layernorm, saber_k_rope, saber_k_softmax_rows
    SAM heads        prompt encoder (no point / mask prompt) + two-way transformer + upscaling on the memory-conditioned embedding
                                                                   saber_set_embed_tokens + saber_decode_points (+ saber_get_decoder_tokens)
    object pointer   3-layer MLP on the chosen mask token           saber_k_gemm_ld
    memory encoder   mask down-sampler, fuser, projection          saber_k_conv3x3s2, saber_k_layernorm (+GELU), saber_k_dwconv7, saber_k_gemm_ld, saber_k_axpy
    masks            up / down-sampling, "mask for memory"          saber_k_resize_plane, saber_k_conv4x4s4
With batch_objects on, the memory attention of a frame's objects runs as one batch (_memory_conditioned_batch) and, with batch_tail, so does
what follows it (_track_tail_batch: saber_k_conv3x3s2_t_batched, saber_k_dwconv7_t_batched, saber_k_gemm_ld_batched, one host wait per frame).

torch is used for device allocation, host<->device copies and a handful of scalar read-backs (argmax of 3 IoU predictions, the sign
of the object score) - the decisions upstream also takes on the host.  Objects are tracked independently, as upstream does.
Settings follow the sam2.1 configs and the reference's construction (num_maskmem truncated to SAM2AdapterConfig.num_maskmem = 2,
predictor.py:28-34).  Upstream's hole filling (fill_holes_in_mask_scores on the low-resolution logits after every single-frame inference;
its default fill_hole_area is 8 where its CUDA extension is built) is VideoPredictor(fill_hole_area=...): saber_k_fill_holes, off (0) by default.
Upstream's non_overlap_masks (_apply_non_overlapping_constraints on the video-resolution logits of every output: at each pixel the first
object with the highest logit keeps its value, the others are clamped to at most -10) is VideoPredictor(non_overlap_masks=True): the resize of
a frame's planes and the constraint are one launch, saber_k_resize_planes_non_overlap (_video_logits); off by default, and nothing that is
stored changes.  non_overlap_masks_for_mem_enc does nothing under upstream's per-object inference (batch 1) and has no counterpart here.
"""
import ctypes as C
import math
import os
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch


NO_OBJ_SCORE = -1024.0
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2


def _bf16_bits(a: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bit patterns, round to nearest even (the engine's weight conversion)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return r.astype(np.uint16)


def _f16_bits(a: np.ndarray) -> np.ndarray:
    """fp32 -> IEEE half bit patterns, round to nearest even (the engine's weight conversion in SABER_PRECISION_FP16)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if np.abs(a).max(initial=0.0) > 65504.0:
        raise ValueError("a memory-model weight exceeds the fp16 range (65504): run this checkpoint with bf16 operands")
    return a.astype(np.float16).view(np.uint16)


class _OperandLib:
    """The kernel-level C-ABI (saber_k_*) with the calling thread's 16-bit operand type set to fp16 around every call
    (include/saber_amd_kernels.h: saber_k_set_operand_type is thread-local; the engine-level entry points set it from the handle)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("saber_k_") or name in ("saber_k_last_error", "saber_k_set_operand_type"):
            return fn
        lib = self._lib

        def call(*args):
            prev = lib.saber_k_set_operand_type(1)
            try:
                return fn(*args)
            finally:
                lib.saber_k_set_operand_type(prev)
        setattr(self, name, call)
        return call


def _sine_pe_2d(side: int, num_pos_feats: int) -> np.ndarray:
    """upstream PositionEmbeddingSine(normalize=True, scale 2 pi, temperature 1e4): (side*side, 2*num_pos_feats), y half first"""
    eps, scale = 1e-6, 2 * math.pi
    yy, xx = np.meshgrid(np.arange(1, side + 1, dtype=np.float32), np.arange(1, side + 1, dtype=np.float32), indexing="ij")
    yy = yy / np.float32(side + eps) * np.float32(scale)
    xx = xx / np.float32(side + eps) * np.float32(scale)
    d = np.arange(num_pos_feats, dtype=np.float32)
    d = np.float32(10000.0) ** (2 * np.floor(d / 2) / np.float32(num_pos_feats))
    px, py = xx[:, :, None] / d, yy[:, :, None] / d
    px = np.stack((np.sin(px[:, :, 0::2]), np.cos(px[:, :, 1::2])), 3).reshape(side, side, -1)
    py = np.stack((np.sin(py[:, :, 0::2]), np.cos(py[:, :, 1::2])), 3).reshape(side, side, -1)
    return np.concatenate((py, px), 2).reshape(side * side, 2 * num_pos_feats).astype(np.float32)


def _sine_pe_1d(pos: np.ndarray, dim: int) -> np.ndarray:
    pe_dim = dim // 2
    dim_t = np.float32(10000.0) ** (2 * np.floor(np.arange(pe_dim, dtype=np.float32) / 2) / np.float32(pe_dim))
    e = pos.astype(np.float32)[:, None] / dim_t
    return np.concatenate([np.sin(e), np.cos(e)], -1).astype(np.float32)


def window_shares(k: int, world: int) -> List[Tuple[int, int]]:
    """[a, b) of the k frames of a window for each of `world` ranks: contiguous, ceil(k / world) frames each until the frames run out
    (the trailing ranks of a short window get nothing)."""
    per = -(-k // world) if k > 0 else 0
    return [(min(k, r * per), min(k, (r + 1) * per)) for r in range(world)]


def bank_signature(st: dict, t: int, reverse: bool, num_maskmem: int, num_frames: int) -> Tuple[tuple, tuple]:
    """What the memory bank of one object looks like on frame t, from its outputs st = {"cond": {frame: ...}, "non_cond": {frame: ...}}
    alone (no device data): (temporal slot of every spatial memory, in bank order; offset of every object pointer, in bank order) - the
    selection rules of VideoPredictor._memory_conditioned.  Objects with equal signatures have banks of one shape with the same position
    rows, so their memory attention can run as one batch."""
    slots = [num_maskmem - 1] * len(st["cond"])
    for t_pos in range(1, num_maskmem):
        t_rel = num_maskmem - t_pos
        if (t + t_rel if reverse else t - t_rel) in st["non_cond"]:
            slots.append(num_maskmem - t_pos - 1)
    max_ptrs = min(num_frames, 16)
    sign = -1 if reverse else 1
    offs = [(t - tc) * sign for tc in st["cond"] if ((tc >= t) if reverse else (tc <= t))]
    for d in range(1, max_ptrs):
        tt = t + d if reverse else t - d
        if tt < 0 or tt >= num_frames:
            break
        if tt in st["non_cond"]:
            offs.append(d)
    return tuple(slots), tuple(offs)


def group_by_signature(oids: List[int], signatures: List[tuple], object_batch: int) -> List[List[int]]:
    """Batches of the objects `oids` (parallel to `signatures`): objects of one signature form a group, in the order of `oids`; groups come in
    the order of their first object; a group larger than object_batch is cut into chunks of at most object_batch."""
    if object_batch < 1:
        raise ValueError("object_batch must be at least 1")
    groups: Dict[tuple, List[int]] = {}
    for oid, sig in zip(oids, signatures):
        groups.setdefault(sig, []).append(oid)
    return [g[i:i + object_batch] for g in groups.values() for i in range(0, len(g), object_batch)]


# One frame in the frame-feature store: what saber_export_slots writes for one slot (image_embed 4096 x 256, feat_s1 16384 x 64, feat_s0
# 65536 x 32), fp32 whatever the handle's operand type: 16 MiB
FRAME_STORE_SIZES = (4096 * 256, 16384 * 64, 65536 * 32)
FRAME_STORE_BYTES = 4 * sum(FRAME_STORE_SIZES)


def frame_store_budget(frame_store_gb: Optional[float] = None) -> int:
    """Bytes the frame-feature store may take: frame_store_gb GiB; None = the environment's SABER_AMD_VIDEO_STORE_GB, else 0 (off)."""
    if frame_store_gb is None:
        frame_store_gb = float(os.environ.get("SABER_AMD_VIDEO_STORE_GB") or 0)
    frame_store_gb = float(frame_store_gb)
    if not frame_store_gb >= 0:
        raise ValueError("frame_store_gb must be non-negative")
    return int(frame_store_gb * 2 ** 30)


def frame_store_rows(budget_bytes: int, num_frames: int) -> int:
    """Frames the store holds: as many whole frames as the budget pays for, at most the volume's own"""
    return max(0, min(int(budget_bytes) // FRAME_STORE_BYTES, int(num_frames)))


def plan_window(t0: int, t1: int, stored, free_rows: int) -> Tuple[List[int], List[int], bool]:
    """How the frame-feature store serves the window [t0, t1): (the window's frames that are not in `stored`, ascending; those of them that
    get one of the `free_rows` rows; whether the window is served from the store).  Rows are allotted first come and never given back, so a
    window is served only when every missing frame gets a row; otherwise it is encoded as a whole, as without the store, and stores nothing."""
    missing = [t for t in range(t0, t1) if t not in stored]
    served = len(missing) <= free_rows
    return missing, (missing if served else []), served


def load_tomogram_frames(tomogram: np.ndarray, image_size: int = 1024, light_modality: bool = False) -> np.ndarray:
    """TomogramPreprocessor as the adapter applies it (saber/adapters/preprocessing.py:27-76 via predictor.py:98-105): min-max to [-1,1],
    per-slice resize to image_size (skimage.transform.resize(anti_aliasing=True): the identity at image_size, order-1 interpolation at
    pixel centres; on a DOWN-sampled axis preceded by the Gaussian anti-aliasing filter of sigma (factor - 1) / 2), then `2x - 1` once more
    (img_mean / img_std are None on this path, so frames span [-3, 1]).  Host glue on the whole volume, like the reference.
    Returns (Z, image_size, image_size) float32: one gray plane per frame (the reference's 3 identical channels)."""
    t = np.asarray(tomogram, dtype=np.float64)
    t = (t - t.min()) / (t.max() - t.min())
    t = t * 2 - 1
    Z, H, W = t.shape
    if (H, W) != (image_size, image_size):
        if H > image_size or W > image_size:
            # skimage.transform.resize(anti_aliasing=True) on a down-sampled axis: Gaussian of sigma = (factor - 1) / 2 (scipy's
            # gaussian_filter, boundary mode 'mirror' = skimage's default 'reflect', truncate 4), then order-1 interpolation at pixel centres
            from scipy import ndimage as ndi
            sig = (max(0.0, (H / image_size - 1) / 2), max(0.0, (W / image_size - 1) / 2))
            t = np.stack([ndi.gaussian_filter(t[z], sig, mode="mirror") for z in range(Z)])
        ys = np.clip((np.arange(image_size) + 0.5) * H / image_size - 0.5, 0, H - 1)
        xs = np.clip((np.arange(image_size) + 0.5) * W / image_size - 0.5, 0, W - 1)
        y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
        y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
        fy, fx = (ys - y0)[None, :, None], (xs - x0)[None, None, :]
        a = t[:, y0][:, :, x0] * (1 - fx) + t[:, y0][:, :, x1] * fx
        b = t[:, y1][:, :, x0] * (1 - fx) + t[:, y1][:, :, x1] * fx
        t = a * (1 - fy) + b * fy
    out = (2 * t.astype(np.float32) - 1).astype(np.float32)
    if light_modality:
        out = (out - out.min()) / (out.max() - out.min()) * 255
    return out


def load_tomogram_frames_device(tomogram, lib, device, image_size: int = 1024, light_modality: bool = False) -> torch.Tensor:
    """load_tomogram_frames on the device: the two affine steps (min-max to [-1,1], then 2x - 1) commute with the bilinear resize, so the
    volume is uploaded once and one resize launch with the fused affine map v -> 4 (v - min) / (max - min) - 3 produces the (Z, 1024, 1024)
    frame stack in HBM (the host version spends ~25 ms per slice in numpy); tomograms larger than 1024 px go through the Gaussian filter first.
    A CUDA float32 tensor (what tomoSegmenter's device preparation hands over) is read where it lies and is not modified."""
    if isinstance(tomogram, torch.Tensor):
        if not tomogram.is_cuda or tomogram.dtype != torch.float32 or tomogram.dim() != 3:
            raise TypeError("load_tomogram_frames_device: a tensor tomogram must be a (Z,H,W) CUDA float32 tensor")
        t = tomogram.to(device).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(tomogram, dtype=np.float32)).to(device)
    Z, H, W = t.shape
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    mn, mx = (float(v) for v in torch.aminmax(t))              # of the tomogram as loaded: the reference normalises before it resizes
    if H > image_size or W > image_size:
        # the Gaussian anti-aliasing of skimage's down-sampling resize (saber_k_gauss_mirror: scipy's gaussian_filter, mode 'mirror'), per
        # down-sampled axis; its taps sum to one, so it commutes with the affine normalisation applied by the resize launch below
        for axis, n in ((0, H), (1, W)):
            sigma = (n / image_size - 1) / 2
            if sigma > 0:
                tmp = torch.empty_like(t)
                if lib.saber_k_gauss_mirror(C.c_void_p(t.data_ptr()), C.c_void_p(tmp.data_ptr()), Z, H, W, axis, float(sigma), stream) != 0:
                    raise RuntimeError(lib.saber_k_last_error().decode())
                t = tmp
    a = 4.0 / (mx - mn)
    out = torch.empty((Z, image_size, image_size), dtype=torch.float32, device=device)
    if lib.saber_k_resize_plane(C.c_void_p(t.data_ptr()), Z, H, W, C.c_void_p(out.data_ptr()), image_size, image_size, 0, 3, a, -a * mn - 3.0, stream) != 0:
        raise RuntimeError(lib.saber_k_last_error().decode())
    if light_modality:
        lo, hi = torch.aminmax(out)
        out = (out - lo) / (hi - lo) * 255
    return out


class VideoPredictor:
    """add_new_mask / propagate_in_video of the SAM2 video predictor on one engine handle."""

    def __init__(self, engine, weights: Dict[str, np.ndarray], num_maskmem: int = 2, batch_objects: Optional[bool] = None, object_batch: int = 16,
                 fill_hole_area: int = 0, batch_tail: Optional[bool] = None, frame_store_gb: Optional[float] = None,
                 non_overlap_masks: Optional[bool] = None):
        """batch_objects: the memory attention of all objects that are tracked on a frame runs as one set of launches
        (_memory_conditioned_batch; bit-identical to the per-object route); None = the environment switch SABER_AMD_VIDEO_BATCH=1, else off.
        object_batch: most objects per batch (bounds the workspace and activations: ~0.1 GB per object)
        fill_hole_area: upstream's setting of the same name (8 in a default upstream build): every 8-connected component of at most that many
        pixels of the background (logit <= 0) of a frame's 256 x 256 logits is set to the logit 0.1 before the frame's output is stored
        (_fill_holes).  0 = off: no launch, nothing allocated.
        batch_tail: read only when batch_objects is on: what follows the memory attention on a tracked frame (SAM heads, object pointers,
        memory encoder, hole fill, the resize of the yield) runs for all of the frame's objects together, with one host wait per frame
        (_track_tail_batch; bit-identical to the per-object tail).  None = on unless SABER_AMD_VIDEO_BATCH_TAIL=0; False = the per-object tail
        behind the batched attention.
        frame_store_gb: GiB of device memory for the frame-feature store: the encoder outputs of a frame (16 MiB of fp32, what
        saber_export_slots writes for a slot) are kept when a window is encoded and copied back (saber_import_slots) when a later window
        needs the frame again - another seed, the other direction, another slab of the same volume - so that a frame goes through the
        encoder once per volume.  Rows = budget // 16 MiB, at most the volume's frames, allocated on first use and allotted first come
        (no eviction): a window with a frame that is neither stored nor can get a row is encoded as a whole, as without the store.  The
        store outlives reset_state(), and init_state() with frames bit-equal to the loaded ones; drop_frame_store() frees it.  Same bits as
        without it.  Bypassed while window encodes shard over ranks (_ranks()[0] > 1).  None = the environment's SABER_AMD_VIDEO_STORE_GB,
        else 0 = off: no launch, nothing allocated.
        non_overlap_masks: upstream's setting of the same name: in every stack of video-resolution logits this class hands out (the yields of
        propagate_in_video, _frame_output) at most one object stays above -10 at a pixel - the first one, in obj_ids order, with the highest
        logit keeps its value, every other one reads min(value, -10) (_video_logits: the resize and the constraint in one launch).  Applied
        after fill_hole_area, to the outputs alone: memories, object pointers and the stored pred_masks are those of a run without it.
        None = the environment switch SABER_AMD_NON_OVERLAP_MASKS=1, else off: no new launch, nothing allocated, the outputs as before."""
        self.non_overlap_masks = os.environ.get("SABER_AMD_NON_OVERLAP_MASKS", "0") not in ("", "0") if non_overlap_masks is None else bool(non_overlap_masks)
        if fill_hole_area < 0:
            raise ValueError("fill_hole_area must be non-negative")
        self.fill_hole_area = int(fill_hole_area)
        self.frame_store_budget = frame_store_budget(frame_store_gb)
        self.encoded_frames = 0          # frames sent through eng.encode since construction (every route)
        self.restored_frames = 0         # frames copied from the store into a slot
        self._store = None               # the three (rows, size) fp32 tensors of FRAME_STORE_SIZES
        self._store_row: Dict[int, int] = {}     # frame -> its row
        self._frames_dev = None
        if num_maskmem > 7:
            raise ValueError("num_maskmem must be at most 7")
        if object_batch < 1:
            raise ValueError("object_batch must be at least 1")
        self.batch_objects = os.environ.get("SABER_AMD_VIDEO_BATCH", "0") not in ("", "0") if batch_objects is None else bool(batch_objects)
        self.object_batch = int(object_batch)
        self.batch_tail = os.environ.get("SABER_AMD_VIDEO_BATCH_TAIL", "1") != "0" if batch_tail is None else bool(batch_tail)
        self.eng, self.lib, self.dev = engine, engine.lib, engine.device
        # 16-bit operand type of the engine handle: every uint16 buffer of this class (GEMM weights, stored memories, attention operands)
        # holds that type's bit patterns
        self.f16 = getattr(engine, "operands", "bf16") == "fp16"
        if self.f16:
            self.lib = _OperandLib(engine.lib)
        if self.lib.saber_k_init(engine.device_index) != 0:
            raise RuntimeError(self.lib.saber_k_last_error().decode())
        self.num_maskmem = num_maskmem
        self.image_size = 1024
        self.shard_encodes = os.environ.get("SABER_AMD_VIDEO_SHARD", "1") != "0"
        # what the sharded window encodes ship through the all-gather: "fp32" (default; 16 MiB per frame, every rank ends up with the bits a
        # single process computes) or "op16" (the three feature arrays rounded to the handle's 16-bit operand type: 8 MiB per frame - SURVEY.md
        # 8f-1 sized the exchange that way; every rank, the encoding one included, then decodes from the ROUNDED features, so the ranks agree
        # bit for bit with each other but not with an unsharded run: +4e-3 (bf16) / +5e-4 (fp16) on the features).  Over xGMI the fp32 gather
        # of a 16-frame window is ~2 ms against ~55 ms of work per window, so precision is the default and bytes are the option.
        # Round 5: on an fp16 handle (the adapter's default) the 16-bit gather is the default - its +5e-4 is inside that mode's 1e-3 budget and the
        # window then moves 8 instead of 16 MiB per frame; bf16 handles keep fp32 (+4e-3 would double that mode's error).
        self.gather_dtype = os.environ.get("SABER_AMD_VIDEO_GATHER", "op16" if getattr(engine, "operands", "bf16") == "fp16" else "fp32")
        if self.gather_dtype not in ("fp32", "op16"):
            raise ValueError("SABER_AMD_VIDEO_GATHER must be 'fp32' or 'op16'")
        self._keep: List[torch.Tensor] = []
        W = weights
        missing = [k for k in ("memory_attention.norm.weight", "memory_encoder.out_proj.weight", "obj_ptr_proj.layers.0.weight", "maskmem_tpos_enc") if k not in W]
        if missing:
            raise ValueError(f"the video path needs the memory-model tensors of the checkpoint; missing {missing}")
        self.f32: Dict[str, torch.Tensor] = {}
        self.bf: Dict[str, torch.Tensor] = {}
        for k, v in W.items():
            if not (k.startswith(("memory_attention.", "memory_encoder.", "obj_ptr_proj.", "obj_ptr_tpos_proj.", "mask_downsample.")) or
                    k in ("maskmem_tpos_enc", "no_obj_ptr", "no_obj_embed_spatial", "no_mem_embed")):
                continue
            a = np.ascontiguousarray(v, dtype=np.float32)
            self.f32[k] = torch.from_numpy(a).to(self.dev)
            is_gemm_w = k.endswith(".weight") and a.ndim >= 2 and "dwconv" not in k and not k.startswith("mask_downsample.") and \
                ("mask_downsampler.encoder" not in k or k.endswith("encoder.12.weight"))
            if is_gemm_w:       # operands of the bf16 MFMA GEMM: [N][K] row-major, bf16 (RNE) like the engine's own weights
                self.bf[k] = torch.from_numpy((_f16_bits if self.f16 else _bf16_bits)(a.reshape(a.shape[0], -1))).to(self.dev)
        self.tpos = np.asarray(W["maskmem_tpos_enc"], dtype=np.float32)[:num_maskmem].reshape(num_maskmem, -1)      # predictor.py:31-32
        self.no_obj_ptr = np.asarray(W["no_obj_ptr"], dtype=np.float32).reshape(1, 256)
        self.no_obj_spatial = np.asarray(W["no_obj_embed_spatial"], dtype=np.float32).reshape(-1)
        self.neg_no_mem = torch.from_numpy(-np.asarray(W["no_mem_embed"], dtype=np.float32).reshape(1, 256)).to(self.dev)
        self.pos_no_mem = torch.from_numpy(np.asarray(W["no_mem_embed"], dtype=np.float32).reshape(1, 256).copy()).to(self.dev)
        self.curr_pos = torch.from_numpy(_sine_pe_2d(64, 128)).to(self.dev)                     # (4096,256)
        self.mem_pos = _sine_pe_2d(64, 32)                                                      # (4096,64)
        # spatial position + temporal encoding of a memory that is k slots away, once per model (device)
        self.mem_pos_t = [torch.from_numpy(self.mem_pos + self.tpos[k][None]).to(self.dev) for k in range(num_maskmem)]
        self.no_obj_ptr_dev = torch.from_numpy(self.no_obj_ptr).to(self.dev)
        self.no_obj_spatial_bias = (self.f32["memory_encoder.out_proj.bias"] + torch.from_numpy(self.no_obj_spatial).to(self.dev)).contiguous()
        # mask down-sampler convolutions with the weights laid out (3,3,Cin,Cout) for saber_k_conv3x3s2_t
        self.conv_t = {j: torch.from_numpy(np.ascontiguousarray(np.asarray(W[f"memory_encoder.mask_downsampler.encoder.{3 * j}.weight"], dtype=np.float32)
                                                                .transpose(2, 3, 1, 0))).to(self.dev) for j in range(4)}
        # depth-wise 7x7 weights of the fuser laid out (49, C) for saber_k_dwconv7_t
        self.dw_t = {i: torch.from_numpy(np.ascontiguousarray(np.asarray(W[f"memory_encoder.fuser.layers.{i}.dwconv.weight"], dtype=np.float32).reshape(256, 49).T)).to(self.dev)
                     for i in range(2)}
        self._pe1d_cache: Dict[tuple, torch.Tensor] = {}
        self._flash_ws = None
        self._flash_ws_batch = None
        self._fill_ws = None             # labels + sizes of saber_k_fill_holes
        self._no_obj_plane = None        # (256,256) of NO_OBJ_SCORE: the logits of an object the heads predict absent (_track_tail_batch)
        self._pad_point = None           # upstream's padding point (0, 0) with label -1, on the device
        self._mem_pos_all = None         # mem_pos_t as one (num_maskmem, 4096, 64) table for saber_k_membank_assemble
        self.hook = None
        self.images = None

    # ------------------------------------------------------------------ small wrappers over the C-ABI
    def _p(self, t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _s(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _ck(self, st):
        if st != 0:
            raise RuntimeError(f"saber_amd: {self.lib.saber_k_last_error().decode()}")

    def _new(self, *shape, dtype=torch.float32, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.dev)

    def _gemm(self, A, Wb, bias, M, N, K, out_f32=None, out_bf=None, res=None, act=ACT_NONE, lda=None, ldw=None):
        """C = act(A[M,K] . W[N,K]^T + bias) (+ res); A, W bf16 (uint16 storage)"""
        self._ck(self.lib.saber_k_gemm_ld(self._p(A), lda or K, self._p(Wb), ldw or K, 1 if (ldw or K) % 64 == 0 else 0, self._p(bias), self._p(res),
                                          self._p(out_f32), self._p(out_bf), M, N, K, act, self._s()))

    def _to_bf(self, x, rows, Cn, y=None, y_rows=1):
        out = self._new(rows, Cn, dtype=torch.uint16)
        self._ck(self.lib.saber_k_add_to_bf16(self._p(x), self._p(y), y_rows, self._p(out), None, rows, Cn, self._s()))
        return out

    def _ln(self, x, key, rows, Cn, eps, bf=True, act=ACT_NONE):
        out = self._new(rows, Cn, dtype=torch.uint16 if bf else torch.float32)
        self._ck(self.lib.saber_k_layernorm(self._p(x), self._p(self.f32[key + ".weight"]), self._p(self.f32[key + ".bias"]), eps,
                                            None if bf else self._p(out), self._p(out) if bf else None, rows, Cn, act, self._s()))
        return out

    def _lin(self, x_bf, key, M, out_bf=False, res=None, act=ACT_NONE, bias=None):
        w = self.bf[key + ".weight"]
        N, K = w.shape
        out = self._new(M, N, dtype=torch.uint16 if out_bf else torch.float32)
        self._gemm(x_bf, w, self.f32[key + ".bias"] if bias is None else bias, M, N, K, None if out_bf else out, out if out_bf else None, res, act)
        return out

    # ------------------------------------------------------------------ state
    def init_state(self, frames, video_hw: Optional[Tuple[int, int]] = None):
        """frames: (Z, 1024, 1024) float32 gray planes as load_tomogram_frames (numpy) or load_tomogram_frames_device (tensor) return them"""
        assert frames.ndim == 3 and tuple(frames.shape[1:]) == (1024, 1024)
        self.images = frames
        self.num_frames = frames.shape[0]
        self.video_hw = video_hw or (1024, 1024)
        self.obj_ids: List[int] = []
        self.out: Dict[int, Dict[str, dict]] = {}
        self.temp: Dict[int, dict] = {}
        self._raw: Dict[int, torch.Tensor] = {}
        self._win = (0, 0)
        if self.frame_store_budget >= FRAME_STORE_BYTES:
            # the store belongs to the frames it was computed from: the stack is uploaded now (a copy of this predictor's own: what the caller
            # does to a device tensor afterwards cannot reach it) and the store survives only if the stack it came from has the same bits
            held, new = self._frames_dev, self._upload_frames()
            if isinstance(frames, torch.Tensor) and new.data_ptr() == frames.data_ptr():
                new = new.clone()
            if held is not None and held.shape == new.shape and torch.equal(held, new):
                new = held
            else:
                self.drop_frame_store()
            self._frames_dev = new
        else:
            self._frames_dev = None
        self._points = {}                # (obj_id, frame_idx) -> (points in model pixels (k,2), labels (k,)): the clicks a frame has accumulated
        self._tracked = {}               # (obj_id, frame_idx) -> reverse flag of the propagation that last went over the frame (upstream: frames_tracked_per_obj)

    def reset_state(self):
        """prompts and tracking results go; the loaded frames and the frame-feature store stay"""
        self.obj_ids, self.out, self.temp, self._raw, self._win = [], {}, {}, {}, (0, 0)
        self._points, self._tracked = {}, {}

    def _upload_frames(self) -> torch.Tensor:
        return (self.images.to(self.dev, dtype=torch.float32).contiguous() if isinstance(self.images, torch.Tensor) else
                torch.from_numpy(np.ascontiguousarray(self.images, dtype=np.float32)).to(self.dev))

    # ------------------------------------------------------------------ frame-feature store
    @property
    def stored_frames(self) -> int:
        """rows of the frame-feature store in use"""
        return len(self._store_row)

    @property
    def store_bytes(self) -> int:
        """device memory the frame-feature store holds now"""
        return 0 if self._store is None else self._store[0].shape[0] * FRAME_STORE_BYTES

    def drop_frame_store(self):
        """frees the frame-feature store; the next window allocates it again"""
        self._store, self._store_row = None, {}

    def _store_ptrs(self, row: int):
        return [C.c_void_p(s.data_ptr() + row * s.shape[1] * 4) for s in self._store]

    def _window_from_store(self, t0: int, t1: int, missing: List[int]):
        """The window [t0, t1) into slots 0..t1-t0-1 through the store (plan_window said it can be served): the missing frames go through the
        encoder as one batched pass into slots 0.., are exported to their rows at once - _sam_heads overwrites a slot's image_embed with the
        memory-conditioned tokens - and every frame that is not yet in its slot is imported.  Bit-identical to encoding the window, because
        the encoder's per-image results do not depend on the batch they ran in (tests/test_gpu_graphs.py) and export / import are copies."""
        rows = frame_store_rows(self.frame_store_budget, self.num_frames)
        if self._store is None:
            self._store = [torch.empty((rows, sz), dtype=torch.float32, device=self.dev) for sz in FRAME_STORE_SIZES]
        m = len(missing)
        if m:
            # crop boxes over the (frames * 1024, 1024) view of the stack from the first to the last missing frame: they need not be contiguous
            a, b = missing[0], missing[-1] + 1
            self.eng.encode(self._frames_dev[a:b].view((b - a) * 1024, 1024), crop_boxes=[[0, (f - a) * 1024, 1024, (f - a + 1) * 1024] for f in missing],
                            slot0=0, normalised_grey=True)
            self.encoded_frames += m
            r0 = len(self._store_row)
            assert r0 + m <= rows
            self.eng._check(self.lib.saber_export_slots(self.eng.h, 0, m, *self._store_ptrs(r0), self._s()))
            for i, f in enumerate(missing):
                self._store_row[f] = r0 + i
        # frame t0 + j belongs in slot j; missing[j] is there already when it is the window's j-th frame.  Runs of consecutive rows are one call
        k = t1 - t0
        todo = [j for j in range(k) if not (j < m and missing[j] == t0 + j)]
        i = 0
        while i < len(todo):
            j, r, n = todo[i], self._store_row[t0 + todo[i]], 1
            while i + n < len(todo) and todo[i + n] == j + n and self._store_row[t0 + j + n] == r + n:
                n += 1
            self.eng._check(self.lib.saber_import_slots(self.eng.h, j, n, *self._store_ptrs(r), self._s()))
            i += n
        self.restored_frames += len(todo)

    def _frame(self, t: int, reverse: bool = False) -> torch.Tensor:
        """RAW top-level features of frame t (without no_mem_embed) as (4096,256) fp32 row-major tokens.  Frames are encoded a WINDOW at a
        time: the per-frame Hiera passes are independent, so the next max_images frames in the direction of travel
        go through the encoder as one batched pass (the device copy of the frame stack is a (Z*1024, 1024) image whose crop boxes are
        the frames) and stay in the engine's slots, where the decoder finds their high-resolution features."""
        if t in self._raw:
            return self._raw[t]
        B = self.eng.max_images
        t0, t1 = (max(0, t - B + 1), t + 1) if reverse else (t, min(self.num_frames, t + B))
        if self._frames_dev is None:
            self._frames_dev = self._upload_frames()
        k = t1 - t0
        world, rank = self._ranks()
        # the frame-feature store is consulted here alone, where a window would be encoded; sharded window encodes bypass it
        rows = frame_store_rows(self.frame_store_budget, self.num_frames) if world == 1 else 0
        missing, _, served = plan_window(t0, t1, self._store_row, rows - len(self._store_row)) if rows else ([], [], False)
        if world > 1:
            self._encode_window_sharded(t0, t1, world, rank)
            a, b = window_shares(k, world)[rank]
            self.encoded_frames += b - a
        elif served:
            self._window_from_store(t0, t1, missing)
        else:
            self.eng.encode(self._frames_dev[t0:t1].view(k * 1024, 1024), crop_boxes=[[0, i * 1024, 1024, (i + 1) * 1024] for i in range(k)],
                            slot0=0, normalised_grey=True)
            self.encoded_frames += k
        self._raw, self._win = {}, (t0, t1)
        for i in range(k):
            emb = self._new(4096, 256)
            self.eng._check(self.lib.saber_get_embed_tokens(self.eng.h, i, self._p(emb), self._s()))
            raw = self._new(4096, 256)
            self._ck(self.lib.saber_k_add_to_bf16(self._p(emb), self._p(self.neg_no_mem), 1, None, self._p(raw), 4096, 256, self._s()))
            self._raw[t0 + i] = raw
        return self._raw[t]

    def _ranks(self) -> Tuple[int, int]:
        """(world size, rank) the window encodes shard over: the default process group when one is initialised with more than one rank and
        sharding is not switched off (shard_encodes=False / SABER_AMD_VIDEO_SHARD=0).  Every rank must then run the same tracking calls on
        the same volume: the chain itself is replicated, only the Hiera passes are divided."""
        import torch.distributed as dist
        if not self.shard_encodes or not dist.is_available() or not dist.is_initialized():
            return 1, 0
        return dist.get_world_size(), dist.get_rank()

    def _encode_window_sharded(self, t0: int, t1: int, world: int, rank: int):
        """the frames of a window are dealt to the ranks in contiguous shares (window_shares), each rank encodes its
        share into slots 0.., exports them, one all-gather per feature array (RCCL; staged through host memory under gloo) brings every
        frame to every rank, and the gathered features are imported into slots 0..k-1 - bit-identical to encoding all k here, because the
        encoder's per-image results do not depend on the batch they ran in (tests/test_gpu_graphs.py)."""
        import torch.distributed as dist
        k = t1 - t0
        shares = window_shares(k, world)
        per = shares[0][1] - shares[0][0]
        a, b = shares[rank]
        n = b - a
        if n > 0:
            self.eng.encode(self._frames_dev[t0 + a:t0 + b].view(n * 1024, 1024), crop_boxes=[[0, i * 1024, 1024, (i + 1) * 1024] for i in range(n)],
                            slot0=0, normalised_grey=True)
        sizes = (4096 * 256, 16384 * 64, 65536 * 32)
        mine = [torch.zeros((per, sz), dtype=torch.float32, device=self.dev) for sz in sizes]
        self.eng._check(self.lib.saber_export_slots(self.eng.h, 0, n, self._p(mine[0]), self._p(mine[1]), self._p(mine[2]), self._s()))
        every = [torch.empty((world * per, sz), dtype=torch.float32, device=self.dev) for sz in sizes]
        on_device = dist.get_backend() == "nccl"
        t16 = None if self.gather_dtype == "fp32" else (torch.float16 if self.f16 else torch.bfloat16)
        for src, dst in zip(mine, every):
            if t16 is not None:                      # 16-bit exchange: the same bytes through a byte view (gloo has no 16-bit collectives)
                src16 = src.to(t16).view(torch.uint8)
                dst16 = torch.empty((dst.shape[0], dst.shape[1] * 2), dtype=torch.uint8, device=self.dev)
                if on_device:
                    dist.all_gather_into_tensor(dst16, src16)
                else:
                    host = torch.empty(dst16.shape, dtype=torch.uint8)
                    dist.all_gather_into_tensor(host, src16.cpu())
                    dst16.copy_(host)
                dst.copy_(dst16.view(t16))
            elif on_device:
                dist.all_gather_into_tensor(dst, src)
            else:
                host = torch.empty(dst.shape, dtype=torch.float32)
                dist.all_gather_into_tensor(host, src.cpu())
                dst.copy_(host)
        # rank r's share sits at rows [r * per, r * per + its length) = frames [r * per, ...) of the window: already in slot order
        self.eng._check(self.lib.saber_import_slots(self.eng.h, 0, k, self._p(every[0]), self._p(every[1]), self._p(every[2]), self._s()))

    def _slot(self, t: int) -> int:
        assert self._win[0] <= t < self._win[1]
        return t - self._win[0]

    # ------------------------------------------------------------------ SAM heads on a given (4096,256) embedding
    def _sam_heads(self, embed_tokens: torch.Tensor, mask_in: Optional[torch.Tensor], multimask: bool, slot: int = 0,
                   point: Optional[Tuple[float, float]] = None, label: int = -1, points=None, labels=None):
        """returns (low (256,256) device fp32, obj logit float, obj_ptr (1,256) device fp32); slot: the engine slot that holds the frame;
        point / label: one click in the model's 1024-px frame (None: upstream's padding point with label -1); points (k,2) / labels (k,),
        k > 1: several clicks / a box's corners (saber_decode_prompts) - on the handle's 16-bit kernels when it has multipoint on
        (Engine(..., multipoint=True): the 16-token route, no precision switch), else in the engine's exact precision mode, which the handle
        must then have been created with (Engine(..., precision="exact"); the production precision is restored afterwards)"""
        self.eng._check(self.lib.saber_set_embed_tokens(self.eng.h, slot, self._p(embed_tokens), self._s()))
        if points is not None and len(points) > 1:
            was = self.eng.precision
            multipoint = getattr(self.eng, "multipoint", False)
            if not multipoint and not getattr(self.eng, "has_exact", was == "exact"):
                raise NotImplementedError("several points / a box per prompt make more than 8 decoder tokens: they are decoded on the 16-bit kernels' "
                                          "16-token route (Engine(..., multipoint=True)) or in the exact precision mode (Engine(..., precision='exact'); "
                                          "it can run in bf16 between such calls: Engine.set_precision)")
            pts = torch.as_tensor(np.asarray(points, np.float32).reshape(1, -1, 2)).to(self.dev)
            lab = torch.as_tensor(np.asarray(labels, np.int32).reshape(1, -1)).to(self.dev)
            if multipoint:
                low, iou, obj = self.eng.decode_prompts(pts, lab, slot=slot, multimask=multimask, mask_input=mask_in)
            else:
                self.eng.set_precision("exact")
                try:
                    low, iou, obj = self.eng.decode_prompts(pts, lab, slot=slot, multimask=multimask, mask_input=mask_in)
                finally:
                    self.eng.set_precision(was)
        else:
            if points is not None and len(points) == 1:
                point, label = (float(points[0][0]), float(points[0][1])), int(labels[0])
            pts = torch.zeros(1, 2, device=self.dev) if point is None else torch.tensor([[float(point[0]), float(point[1])]], dtype=torch.float32, device=self.dev)
            lab = torch.full((1,), -1 if point is None else int(label), dtype=torch.int32, device=self.dev)
            low, iou, obj = self.eng.decode_points(pts, slot=slot, multimask=multimask, mask_input=mask_in, labels=lab)
        toks = self._new(8, 256)
        self.eng._check(self.lib.saber_get_decoder_tokens(self.eng.h, 1, self._p(toks), self._s()))
        host = torch.cat([obj.reshape(-1)[:1], iou[0].reshape(-1)]).cpu()       # the one synchronisation of a tracked frame: object score + IoUs
        self.eng.check_finite()          # overflow sentinel of the 16-bit modes (the stream has just drained: a 16-byte copy); SaberRangeError, never NaN masks
        obj_v = float(host[0])
        if self.hook is not None:
            self.hook(obj_v)
        if multimask:
            best = int(torch.argmax(host[1:]))
            low_b, tok = low[0, best], toks[3 + best:4 + best]
        else:
            low_b, tok = low[0, 0], toks[2:3]
        appearing = obj_v > 0
        if appearing:
            h = self._lin(self._to_bf(tok, 1, 256), "obj_ptr_proj.layers.0", 1, out_bf=True, act=ACT_RELU)
            h = self._lin(h, "obj_ptr_proj.layers.1", 1, out_bf=True, act=ACT_RELU)
            ptr = self._lin(h, "obj_ptr_proj.layers.2", 1)                       # (1,256) fp32, stays on the device
        else:
            low_b = torch.full((256, 256), NO_OBJ_SCORE, device=self.dev)
            ptr = self.no_obj_ptr_dev
        return low_b.contiguous(), obj_v, ptr

    def _resize(self, x, H, W, Ho, Wo, antialias=0, post=0, a=0.0, c=0.0):
        out = self._new(Ho, Wo)
        self._ck(self.lib.saber_k_resize_plane(self._p(x), 1, H, W, self._p(out), Ho, Wo, antialias, post, a, c, self._s()))
        return out

    def _fill_holes(self, low: torch.Tensor) -> torch.Tensor:
        """upstream fill_holes_in_mask_scores(pred_masks, fill_hole_area) on (..., 256, 256) logits: a new tensor (what has read `low` before
        keeps the unfilled bits); `low` itself when the step is off"""
        if self.fill_hole_area <= 0:
            return low
        low = low.contiguous()
        need = low.numel() * 8
        if self._fill_ws is None or self._fill_ws.numel() < need:
            self._fill_ws = None
            self._fill_ws = self._new(need, dtype=torch.uint8)
        out = torch.empty_like(low)
        self._ck(self.lib.saber_k_fill_holes(self._p(low), low.numel() // 65536, 256, 256, self.fill_hole_area, 0.1, self._p(out), self._p(self._fill_ws),
                                             self._fill_ws.numel(), self._s()))
        return out

    # ------------------------------------------------------------------ memory encoder
    def _encode_memory(self, raw: torch.Tensor, mask_for_mem: torch.Tensor, appearing: bool):
        """raw (4096,256) fp32 frame features, mask_for_mem (1024,1024) fp32 already scaled (sigmoid or binary, * 20 - 10).
        Returns the spatial memory (4096,64) as stored: bf16 bits."""
        x, H, Cin = mask_for_mem, 1024, 1
        pre = "memory_encoder.mask_downsampler.encoder."
        for j in range(4):
            Cout = Cin * 4
            y = self._new((H // 2) * (H // 2), Cout)
            self._ck(self.lib.saber_k_conv3x3s2_t(self._p(x), H, H, Cin, self._p(self.conv_t[j]), self._p(self.f32[f"{pre}{3 * j}.bias"]), Cout, self._p(y), self._s()))
            H //= 2
            x = self._ln(y, f"{pre}{3 * j + 1}", H * H, Cout, 1e-6, bf=(j == 3), act=ACT_GELU)
            Cin = Cout
        m = self._lin(x, pre + "12", 4096)                                                  # 1x1 conv 256 -> 256
        p = self._lin(self._to_bf(raw, 4096, 256), "memory_encoder.pix_feat_proj", 4096, res=m)
        for i in range(2):
            f = f"memory_encoder.fuser.layers.{i}."
            h = self._new(4096, 256)
            self._ck(self.lib.saber_k_dwconv7_t(self._p(p), 64, 64, 256, self._p(self.dw_t[i]), self._p(self.f32[f + "dwconv.bias"]), self._p(h), self._s()))
            hn = self._ln(h, f + "norm", 4096, 256, 1e-6)
            h1 = self._lin(hn, f + "pwconv1", 4096, out_bf=True, act=ACT_GELU)
            h2 = self._lin(h1, f + "pwconv2", 4096)
            p2 = self._new(4096, 256)
            self._ck(self.lib.saber_k_axpy(self._p(p), self._p(h2), self._p(self.f32[f + "gamma"]), 1.0, 4096, 256, self._p(p2), self._s()))
            p = p2
        # no_obj_embed_spatial on frames where the object is predicted absent
        bias = self.f32["memory_encoder.out_proj.bias"] if appearing else self.no_obj_spatial_bias
        return self._lin(self._to_bf(p, 4096, 256), "memory_encoder.out_proj", 4096, out_bf=True, bias=bias)

    def _encode_memory_batch(self, raw: torch.Tensor, mfm: torch.Tensor, appearing: int) -> torch.Tensor:
        """_encode_memory for the B objects of a tracked frame in one set of launches: raw (4096,256) fp32 frame features (shared), mfm
        (B,1024,1024) fp32 masks for memory, the first `appearing` of them of objects the heads predict present and the rest of absent ones
        (out_proj adds its bias before the 16-bit rounding, so the two groups are two launches).  Returns (B,4096,64) 16-bit storage, block i =
        what _encode_memory returns for object i, bit for bit: the convolutions are the batched forms of the same kernels, LayerNorm / axpy /
        the 16-bit conversion work row by row, and the GEMMs run with the batch dimension of saber_k_gemm_ld_batched."""
        B = mfm.shape[0]
        x, H, Cin = mfm, 1024, 1
        pre = "memory_encoder.mask_downsampler.encoder."
        for j in range(4):
            Cout, Ho = Cin * 4, H // 2
            y = self._new(B, Ho * Ho, Cout)
            self._ck(self.lib.saber_k_conv3x3s2_t_batched(self._p(x), H * H * Cin, H, H, Cin, self._p(self.conv_t[j]), self._p(self.f32[f"{pre}{3 * j}.bias"]), Cout,
                                                          self._p(y), Ho * Ho * Cout, B, self._s()))
            H = Ho
            x = self._ln(y, f"{pre}{3 * j + 1}", B * H * H, Cout, 1e-6, bf=(j == 3), act=ACT_GELU)
            Cin = Cout
        R = 4096 * 256
        m = self._gemm_b(x, R, pre + "12", B, 4096)                                          # 1x1 conv 256 -> 256
        p = self._gemm_b(self._to_bf(raw, 4096, 256), 0, "memory_encoder.pix_feat_proj", B, 4096, res=m, stride_res=R)      # the frame's features: shared
        for i in range(2):
            f = f"memory_encoder.fuser.layers.{i}."
            h = self._new(B, 4096, 256)
            self._ck(self.lib.saber_k_dwconv7_t_batched(self._p(p), R, 64, 64, 256, self._p(self.dw_t[i]), self._p(self.f32[f + "dwconv.bias"]), self._p(h), R, B, self._s()))
            hn = self._ln(h, f + "norm", B * 4096, 256, 1e-6)
            h1 = self._gemm_b(hn, R, f + "pwconv1", B, 4096, out_bf=True, act=ACT_GELU)
            h2 = self._gemm_b(h1, 4096 * 1024, f + "pwconv2", B, 4096)
            p2 = self._new(B, 4096, 256)
            self._ck(self.lib.saber_k_axpy(self._p(p), self._p(h2), self._p(self.f32[f + "gamma"]), 1.0, B * 4096, 256, self._p(p2), self._s()))
            p = p2
        pb = self._to_bf(p, B * 4096, 256).view(B, 4096, 256)
        out = self._new(B, 4096, 64, dtype=torch.uint16)
        for a, b, bias in ((0, appearing, True), (appearing, B, self.no_obj_spatial_bias)):
            if b > a:
                self._gemm_b(pb[a:], R, "memory_encoder.out_proj", b - a, 4096, out_bf=True, bias=bias, out=out[a:], stride_out=4096 * 64)
        return out

    # ------------------------------------------------------------------ prompts
    @torch.inference_mode()
    def add_new_mask(self, frame_idx: int, obj_id: int, mask: np.ndarray):
        """upstream add_new_mask: the mask becomes this frame's output as it is (+-10 logits), its object pointer comes from the SAM heads
        prompted with the mask; the memory of the frame is encoded by the preflight of the next propagate_in_video."""
        if self.images is None:
            raise RuntimeError("call init_state() first")
        if obj_id not in self.obj_ids:
            self.obj_ids.append(obj_id)
            self.out[obj_id] = {"cond": {}, "non_cond": {}}
            self.temp[obj_id] = {}
        m = np.ascontiguousarray(np.squeeze(np.asarray(mask)), dtype=np.float32)
        md = torch.from_numpy(m).to(self.dev)
        if m.shape != (1024, 1024):
            md = self._resize(md, m.shape[0], m.shape[1], 1024, 1024, antialias=1, post=4, a=0.5)
        appearing = bool((md > 0).any().item())
        raw = self._frame(frame_idx)
        high = self._resize(md, 1024, 1024, 1024, 1024, post=3, a=20.0, c=-10.0)
        low = self._resize(high, 1024, 1024, 256, 256, antialias=1)
        mdown = self._new(256, 256)
        self._ck(self.lib.saber_k_conv4x4s4(self._p(md), 1024, 1024, self._p(self.f32["mask_downsample.weight"]), self._p(self.f32["mask_downsample.bias"]), self._p(mdown), self._s()))
        _, _, ptr = self._sam_heads(raw, mdown.view(1, 256, 256), multimask=False, slot=self._slot(frame_idx))
        # the pointer has been through the decoder's own object score (_forward_sam_heads); upstream then blends once more with the
        # appearance the MASK itself says (_use_mask_as_output)
        tok_ptr = ptr if appearing else self.no_obj_ptr_dev
        low = self._fill_holes(low)
        self.temp[obj_id][frame_idx] = {"pred_masks": low, "obj_ptr": tok_ptr, "obj": 10.0 if appearing else -10.0, "mem": None, "raw": raw}
        return frame_idx, list(self.obj_ids), low

    @torch.inference_mode()
    def add_new_points_or_box(self, frame_idx: int, obj_id: int, points=None, labels=None, clear_old_points: bool = True,
                              normalize_coords: bool = True, box=None):
        """upstream SAM2VideoPredictor.add_new_points_or_box on a frame that has not been tracked yet: the SAM heads run on the frame's own
        features (+ no_mem_embed: an initial conditioning frame sees no memory) with the accumulated clicks as the point prompt and the
        frame's previous output, if any, as the mask prompt (clamped to +-32).  A box is its two corners with labels 2 / 3 in front of the
        clicks (only with clear_old_points, as upstream); clicks accumulate over calls unless clear_old_points.  At most one point =>
        multimask output, the best mask by predicted IoU becomes the frame's output (the production bf16 decoder: 8 tokens per prompt);
        more points (or a box) => the single-mask output with dynamic selection, decoded in the engine's exact precision mode (the handle
        must have been created with precision="exact").  On a frame a propagation has already gone over the call is a CORRECTION, as upstream:
        the frame's features are conditioned on the memory bank (in the direction the frame was tracked), its previous output is the mask
        prompt, and the new output replaces the frame's tracked (non-conditioning) output at the next propagation's preflight."""
        if self.images is None:
            raise RuntimeError("call init_state() first")
        if (points is not None) != (labels is not None):
            raise ValueError("points and labels must be provided together")
        if points is None and box is None:
            raise ValueError("at least one of points or box must be provided as input")
        pts = np.zeros((0, 2), np.float32) if points is None else np.asarray(points, dtype=np.float32).reshape(-1, 2)
        lab = np.zeros((0,), np.int32) if labels is None else np.asarray(labels).reshape(-1).astype(np.int32)
        if len(pts) != len(lab):
            raise ValueError("points and labels must have the same length")
        if box is not None:
            if not clear_old_points:
                raise ValueError("cannot add box without clearing old points, since box prompt must be provided before any point prompt "
                                 "(please use clear_old_points=True instead)")
            pts = np.concatenate([np.asarray(box, np.float32).reshape(2, 2), pts], 0)
            lab = np.concatenate([np.array([2, 3], np.int32), lab], 0)
        if obj_id not in self.obj_ids:
            self.obj_ids.append(obj_id)
            self.out[obj_id] = {"cond": {}, "non_cond": {}}
            self.temp[obj_id] = {}
        Hv, Wv = self.video_hw
        xy = pts / np.array([Wv, Hv], np.float32) if normalize_coords else pts
        xy = (xy * np.float32(self.image_size)).astype(np.float32)
        held = self.__dict__.setdefault("_points", {})
        old = None if clear_old_points else held.get((obj_id, frame_idx))
        if old is not None:
            xy, lab = np.concatenate([old[0], xy], 0), np.concatenate([old[1], lab], 0)
        if len(xy) > 9:
            raise NotImplementedError("at most 9 points per object and frame (16 decoder tokens)")
        held[(obj_id, frame_idx)] = (xy, lab)
        # a frame a propagation has already gone over is CORRECTED (upstream: is_init_cond_frame False): features conditioned on the memory bank
        # in the direction the frame was tracked, and the new output stays a non-conditioning one (add_all_frames_to_correct_as_cond False)
        is_init = (obj_id, frame_idx) not in self._tracked
        prev = self.temp[obj_id].get(frame_idx) or self.out[obj_id]["cond"].get(frame_idx) or self.out[obj_id]["non_cond"].get(frame_idx)
        mask_in = prev["pred_masks"].clamp(-32.0, 32.0).view(1, 256, 256).contiguous() if prev is not None else None
        reverse = False if is_init else self._tracked[(obj_id, frame_idx)]
        raw = self._frame(frame_idx, reverse)
        if is_init:
            emb = self._new(4096, 256)
            self._ck(self.lib.saber_k_add_to_bf16(self._p(raw), self._p(self.pos_no_mem), 1, None, self._p(emb), 4096, 256, self._s()))
        else:
            emb = self._memory_conditioned(obj_id, frame_idx, raw, reverse)
        low, obj_v, ptr = self._sam_heads(emb, mask_in, multimask=len(xy) <= 1, slot=self._slot(frame_idx), points=xy, labels=lab)
        low = self._fill_holes(low)          # stored filled: the preflight's memory mask and a later click's mask prompt see the filled logits
        self.temp[obj_id][frame_idx] = {"pred_masks": low, "obj_ptr": ptr, "obj": obj_v, "mem": None, "raw": raw, "is_cond": is_init}
        return frame_idx, list(self.obj_ids), self._resize(low, 256, 256, Hv, Wv)[None, None]

    NO_OBJ_SCORE = -1024.0

    def _frame_output(self, frame_idx: int):
        """(frame_idx, obj_ids, video-resolution mask logits (n_obj,1,Hv,Wv)) of the frame as the state holds it now: an object without an
        output on the frame reads NO_OBJ_SCORE, like upstream's consolidated outputs.  With non_overlap_masks the constraint runs over the
        objects that have an output (_video_logits) and the absent ones are put between them as constant planes: a plane of NO_OBJ_SCORE
        lies below -10, so the clamp leaves it as it is whether it wins or loses, and it wins only where every present object is below it,
        where the clamp leaves those unchanged too - the stack is what the constraint over all n planes gives."""
        Hv, Wv = self.video_hw
        if self.non_overlap_masks:
            held = [self.temp[oid].get(frame_idx) or self.out[oid]["cond"].get(frame_idx) or self.out[oid]["non_cond"].get(frame_idx) for oid in self.obj_ids]
            at = [i for i, o in enumerate(held) if o is not None]
            masks = torch.full((len(held), 1, Hv, Wv), self.NO_OBJ_SCORE, dtype=torch.float32, device=self.dev)
            if at:
                masks[at, 0] = self._video_logits(torch.stack([held[i]["pred_masks"] for i in at], 0), Hv, Wv)
            return frame_idx, list(self.obj_ids), masks
        outs = []
        for oid in self.obj_ids:
            o = self.temp[oid].get(frame_idx) or self.out[oid]["cond"].get(frame_idx) or self.out[oid]["non_cond"].get(frame_idx)
            if o is None:
                outs.append(torch.full((Hv, Wv), self.NO_OBJ_SCORE, dtype=torch.float32, device=self.dev))
            else:
                outs.append(self._resize(o["pred_masks"], 256, 256, Hv, Wv))
        masks = torch.stack(outs, 0)[:, None] if outs else torch.empty((0, 1, Hv, Wv), dtype=torch.float32, device=self.dev)
        return frame_idx, list(self.obj_ids), masks

    @torch.inference_mode()
    def clear_all_prompts_in_frame(self, frame_idx: int, obj_id: int, need_output: bool = True):
        """upstream SAM2VideoPredictor.clear_all_prompts_in_frame: the object's inputs on the frame go; if the frame was a conditioning frame
        its output is kept as a plain tracked (non-conditioning) output, since it no longer receives inputs."""
        if obj_id not in self.obj_ids:
            raise RuntimeError(f"Cannot clear prompts for object id {obj_id}: it does not exist. All existing object ids: {self.obj_ids}.")
        self.temp[obj_id].pop(frame_idx, None)
        self.__dict__.setdefault("_points", {}).pop((obj_id, frame_idx), None)
        out = self.out[obj_id]["cond"].pop(frame_idx, None)
        if out is not None:
            self.out[obj_id]["non_cond"][frame_idx] = out
        if not need_output:
            return None
        return self._frame_output(frame_idx)

    @torch.inference_mode()
    def remove_object(self, obj_id: int, strict: bool = False, need_output: bool = True):
        """upstream SAM2VideoPredictor.remove_object: the object leaves the tracking state at any time.  Returns (remaining object ids,
        [(frame_idx, video-resolution masks of the remaining objects) for every frame the removed object had received inputs on])."""
        if obj_id not in self.obj_ids:
            if not strict:
                return list(self.obj_ids), []
            raise RuntimeError(f"Cannot remove object id {obj_id}: it does not exist. All existing object ids: {self.obj_ids}.")
        input_frames = sorted(set(self.temp[obj_id]) | set(self.out[obj_id]["cond"]))
        self.obj_ids.remove(obj_id)
        self.out.pop(obj_id, None)
        self.temp.pop(obj_id, None)
        self._points = {k: v for k, v in self.__dict__.get("_points", {}).items() if k[0] != obj_id}
        self._tracked = {k: v for k, v in self._tracked.items() if k[0] != obj_id}
        if not need_output or not self.obj_ids:
            return list(self.obj_ids), []
        return list(self.obj_ids), [(t, self._frame_output(t)[2]) for t in input_frames]

    def _preflight(self):
        for oid in self.obj_ids:
            for t, o in self.temp[oid].items():
                if o["mem"] is None:
                    mfm = self._resize(o["pred_masks"], 256, 256, 1024, 1024, antialias=0, post=2, a=20.0, c=-10.0)     # binarised: is_mask_from_pts
                    o["mem"] = self._encode_memory(o["raw"], mfm, o["obj"] > 0)
                    o["raw"] = None
                if o.pop("is_cond", True):
                    self.out[oid]["cond"][t] = o
                else:
                    self.out[oid]["non_cond"][t] = o
            for t in self.out[oid]["cond"]:              # upstream keeps the two dictionaries disjoint (a corrected conditioning frame keeps its old output)
                self.out[oid]["non_cond"].pop(t, None)
            self.temp[oid] = {}
            if not self.out[oid]["cond"]:
                raise RuntimeError("No input points or masks are provided for any object; please add inputs first.")

    # ------------------------------------------------------------------ memory attention
    def _memory_conditioned(self, oid: int, t: int, raw: torch.Tensor, reverse: bool) -> torch.Tensor:
        st = self.out[oid]
        mems, pos = [], []
        for tc, o in st["cond"].items():
            mems.append(o["mem"]); pos.append(self.mem_pos_t[self.num_maskmem - 1])
        for t_pos in range(1, self.num_maskmem):
            t_rel = self.num_maskmem - t_pos
            o = st["non_cond"].get(t + t_rel if reverse else t - t_rel)
            if o is None:
                continue
            mems.append(o["mem"]); pos.append(self.mem_pos_t[self.num_maskmem - t_pos - 1])
        max_ptrs = min(self.num_frames, 16)
        sign = -1 if reverse else 1
        offs, ptrs = [], []
        for tc, o in st["cond"].items():
            if (tc >= t) if reverse else (tc <= t):
                offs.append((t - tc) * sign); ptrs.append(o["obj_ptr"])
        for d in range(1, max_ptrs):
            tt = t + d if reverse else t - d
            if tt < 0 or tt >= self.num_frames:
                break
            o = st["non_cond"].get(tt)
            if o is not None:
                offs.append(d); ptrs.append(o["obj_ptr"])
        n_spatial = 4096 * len(mems)
        n_ptr_tok = 4 * len(ptrs)
        Nk = n_spatial + n_ptr_tok
        Nkp = (Nk + 63) // 64 * 64
        # memory tokens (bf16 as stored) and their position encodings (fp32): [spatial memories ..., pointer tokens], assembled on the device
        mem_bf = self._new(Nkp, 64, dtype=torch.uint16, zero=True)
        pos_d = self._new(Nk, 64)
        for i, (mm, pp) in enumerate(zip(mems, pos)):
            mem_bf[4096 * i:4096 * (i + 1)].copy_(mm)
            pos_d[4096 * i:4096 * (i + 1)].copy_(pp)
        if ptrs:
            P = torch.cat(ptrs, 0).contiguous()                                                # (n,256) fp32, device
            # pointer tokens enter the bank in fp32 upstream; the GEMM operand is bf16 either way
            mem_bf[n_spatial:Nk].copy_(self._to_bf(P, len(ptrs), 256).view(4 * len(ptrs), 64))
            key = (tuple(offs), max_ptrs)
            pe_bf = self._pe1d_cache.get(key)
            if pe_bf is None:
                pe = _sine_pe_1d(np.asarray(offs, np.float32) / np.float32(max_ptrs - 1), 256)
                pe_bf = self._to_bf(torch.from_numpy(pe).to(self.dev), len(ptrs), 256)
                if len(self._pe1d_cache) < 256:
                    self._pe1d_cache[key] = pe_bf
            pe_d = self._lin(pe_bf, "obj_ptr_tpos_proj", len(ptrs))                           # (n,64)
            pos_d[n_spatial:].copy_(pe_d.repeat_interleave(4, dim=0))
        mem_f = self._new(Nk, 64)
        self._ck(self.lib.saber_k_bf16_to_f32(self._p(mem_bf), Nk * 64, self._p(mem_f), self._s()))
        kin_bf = self._to_bf(mem_f, Nk, 64, pos_d, Nk)                                          # bf16(memory + position)
        # ---- 4 layers
        x = self._new(4096, 256)
        self._ck(self.lib.saber_k_axpy(self._p(raw), self._p(self.curr_pos), None, 0.1, 4096, 256, self._p(x), self._s()))
        scale = 1.0 / 16.0

        def attend(q_bf, k_bf, v_bf, n_keys, bv):
            # flash-style (csrc/flash256.hip): no materialised (4096, n_keys) scores; the value bias is added after the product (softmax
            # rows sum to 1)
            O = self._new(4096, 256, dtype=torch.uint16)
            if self._flash_ws is None:
                self._flash_ws = self._new(64 * 8 * 64 * 258)
            self._ck(self.lib.saber_k_flash256(self._p(q_bf), self._p(k_bf), self._p(v_bf), 4096, n_keys, scale, self._p(bv), self._p(O),
                                               self._p(self._flash_ws), self._flash_ws.numel(), self._s()))
            return O

        def rope(x_f32, rows, n_rot):
            out = self._new(rows, 256, dtype=torch.uint16)
            self._ck(self.lib.saber_k_rope(self._p(x_f32), rows, n_rot, 256, 64, 10000.0, None, self._p(out), self._s()))
            return out

        for i in range(4):
            L = f"memory_attention.layers.{i}."
            tb = self._ln(x, L + "norm1", 4096, 256, 1e-5)
            q = rope(self._lin(tb, L + "self_attn.q_proj", 4096), 4096, 4096)
            k = rope(self._lin(tb, L + "self_attn.k_proj", 4096), 4096, 4096)
            v = self._new(4096, 256, dtype=torch.uint16)
            self._gemm(tb, self.bf[L + "self_attn.v_proj.weight"], None, 4096, 256, 256, out_bf=v)
            O = attend(q, k, v, 4096, self.f32[L + "self_attn.v_proj.bias"])
            x = self._lin(O, L + "self_attn.out_proj", 4096, res=x)
            tb = self._ln(x, L + "norm2", 4096, 256, 1e-5)
            q = rope(self._lin(tb, L + "cross_attn_image.q_proj", 4096), 4096, 4096)
            kf = self._new(Nkp, 256, zero=True)
            self._gemm(kin_bf, self.bf[L + "cross_attn_image.k_proj.weight"], self.f32[L + "cross_attn_image.k_proj.bias"], Nk, 256, 64, out_f32=kf)
            k = rope(kf, Nkp, n_spatial)
            v = self._new(Nk, 256, dtype=torch.uint16)
            self._gemm(mem_bf, self.bf[L + "cross_attn_image.v_proj.weight"], None, Nk, 256, 64, out_bf=v)
            O = attend(q, k, v, Nk, self.f32[L + "cross_attn_image.v_proj.bias"])
            x = self._lin(O, L + "cross_attn_image.out_proj", 4096, res=x)
            tb = self._ln(x, L + "norm3", 4096, 256, 1e-5)
            h = self._lin(tb, L + "linear1", 4096, out_bf=True, act=ACT_RELU)
            x = self._lin(h, L + "linear2", 4096, res=x)
        return self._ln(x, "memory_attention.norm", 4096, 256, 1e-5, bf=False)

    # ------------------------------------------------------------------ memory attention of all objects of a frame
    def _gemm_b(self, A, strideA, key, B, M, out_bf=False, res=None, stride_res=0, act=ACT_NONE, bias=True, out=None, stride_out=None):
        """saber_k_gemm_ld for B objects in one launch (the GEMM's batch dimension: every object keeps its own M, so the kernel and the
        summation order are those of _lin / _gemm on one object).  out (optional): a buffer of B blocks of stride_out elements;
        bias: True = the layer's own, False = none, a tensor = that one"""
        w = self.bf[key + ".weight"]
        N, K = w.shape
        if out is None:
            out, stride_out = self._new(B, M, N, dtype=torch.uint16 if out_bf else torch.float32), M * N
        bias_t = self.f32[key + ".bias"] if bias is True else None if bias is False else bias
        self._ck(self.lib.saber_k_gemm_ld_batched(self._p(A), K, strideA, self._p(w), K, 1 if K % 64 == 0 else 0, self._p(bias_t),
                                                  self._p(res), stride_res, None if out_bf else self._p(out), 0 if out_bf else stride_out,
                                                  self._p(out) if out_bf else None, stride_out if out_bf else 0, M, N, K, act, B, self._s()))
        return out

    def _memory_conditioned_group(self, oids: List[int], t: int, reverse: bool, self0: dict) -> torch.Tensor:
        """_memory_conditioned for objects of ONE bank signature: (len(oids), 4096, 256) fp32.  self0: layer 0 up to the cross attention's
        queries, which does not depend on the object (_memory_conditioned_batch computes it once per frame)."""
        B = len(oids)
        slots, offs = bank_signature(self.out[oids[0]], t, reverse, self.num_maskmem, self.num_frames)
        n_mem, n_ptr = len(slots), len(offs)
        mems, ptrs = [], []
        for oid in oids:                                   # the entries bank_signature counted, in its order
            st = self.out[oid]
            mems += [o["mem"] for o in st["cond"].values()]
            for t_pos in range(1, self.num_maskmem):
                t_rel = self.num_maskmem - t_pos
                o = st["non_cond"].get(t + t_rel if reverse else t - t_rel)
                if o is not None:
                    mems.append(o["mem"])
            cond_ptrs = [o["obj_ptr"] for tc, o in st["cond"].items() if ((tc >= t) if reverse else (tc <= t))]
            ptrs += cond_ptrs + [st["non_cond"][t + d if reverse else t - d]["obj_ptr"] for d in offs[len(cond_ptrs):]]
        assert len(mems) == B * n_mem and len(ptrs) == B * n_ptr
        n_spatial, n_ptr_tok = 4096 * n_mem, 4 * n_ptr
        Nk = n_spatial + n_ptr_tok
        Nkp = (Nk + 63) // 64 * 64
        max_ptrs = min(self.num_frames, 16)
        tok = pe4 = None
        if n_ptr:
            # pointer tokens of all objects in one conversion; their position rows depend on the offsets alone: once per group
            tok = self._to_bf(torch.cat(ptrs, 0).contiguous(), B * n_ptr, 256)                  # (B, 4 n_ptr, 64) 16-bit
            key = (tuple(offs), max_ptrs)
            pe_bf = self._pe1d_cache.get(key)
            if pe_bf is None:
                pe = _sine_pe_1d(np.asarray(offs, np.float32) / np.float32(max_ptrs - 1), 256)
                pe_bf = self._to_bf(torch.from_numpy(pe).to(self.dev), n_ptr, 256)
                if len(self._pe1d_cache) < 256:
                    self._pe1d_cache[key] = pe_bf
            pe4 = self._lin(pe_bf, "obj_ptr_tpos_proj", n_ptr).repeat_interleave(4, dim=0).contiguous()      # (4 n_ptr, 64) fp32
        if self._mem_pos_all is None:
            self._mem_pos_all = torch.stack(self.mem_pos_t, 0).contiguous()
        mem_bf = self._new(B, Nkp, 64, dtype=torch.uint16)
        kin_bf = self._new(B, Nkp, 64, dtype=torch.uint16)
        mem_ptrs = (C.c_void_p * max(1, B * n_mem))(*[m.data_ptr() for m in mems])
        pos_idx = (C.c_int * max(1, B * n_mem))(*(list(slots) * B))
        self._ck(self.lib.saber_k_membank_assemble(mem_ptrs, pos_idx, n_mem, self._p(self._mem_pos_all), self.num_maskmem, self._p(tok), n_ptr_tok * 64,
                                                   self._p(pe4), 0, n_ptr_tok, B, self._p(mem_bf), self._p(kin_bf), self._s()))
        scale = 1.0 / 16.0
        R = 4096 * 256

        def attend(q_bf, q_stride, k_bf, k_stride, v_bf, v_stride, n_keys, bv):
            O = self._new(B, 4096, 256, dtype=torch.uint16)
            need = B * 64 * 8 * 64 * 258
            if self._flash_ws_batch is None or self._flash_ws_batch.numel() < need:
                self._flash_ws_batch = None
                self._flash_ws_batch = self._new(need)
            self._ck(self.lib.saber_k_flash256_batched(self._p(q_bf), q_stride, self._p(k_bf), k_stride, self._p(v_bf), v_stride, 4096, n_keys, B, scale,
                                                       self._p(bv), self._p(O), R, self._p(self._flash_ws_batch), self._flash_ws_batch.numel(), self._s()))
            return O

        def rope(x_f32, rows_per, n_rot):
            out = self._new(B, rows_per, 256, dtype=torch.uint16)
            self._ck(self.lib.saber_k_rope_batched(self._p(x_f32), rows_per, B, n_rot, 256, 64, 10000.0, None, self._p(out), self._s()))
            return out

        x = None
        for i in range(4):
            L = f"memory_attention.layers.{i}."
            if i == 0:
                x_res, res_stride, q, q_stride = self0["x"], 0, self0["q"], 0
            else:
                tb = self._ln(x, L + "norm1", B * 4096, 256, 1e-5)
                q = rope(self._gemm_b(tb, R, L + "self_attn.q_proj", B, 4096), 4096, 4096)
                k = rope(self._gemm_b(tb, R, L + "self_attn.k_proj", B, 4096), 4096, 4096)
                v = self._gemm_b(tb, R, L + "self_attn.v_proj", B, 4096, out_bf=True, bias=False)
                O = attend(q, R, k, R, v, R, 4096, self.f32[L + "self_attn.v_proj.bias"])
                x = self._gemm_b(O, R, L + "self_attn.out_proj", B, 4096, res=x, stride_res=R)
                tb = self._ln(x, L + "norm2", B * 4096, 256, 1e-5)
                q, q_stride = rope(self._gemm_b(tb, R, L + "cross_attn_image.q_proj", B, 4096), 4096, 4096), R
                x_res, res_stride = x, R
            kf = self._new(B, Nkp, 256, zero=True)
            self._gemm_b(kin_bf, Nkp * 64, L + "cross_attn_image.k_proj", B, Nk, out=kf, stride_out=Nkp * 256)
            k = rope(kf, Nkp, n_spatial)
            v = self._new(B, Nkp, 256, dtype=torch.uint16)
            self._gemm_b(mem_bf, Nkp * 64, L + "cross_attn_image.v_proj", B, Nk, out_bf=True, bias=False, out=v, stride_out=Nkp * 256)
            O = attend(q, q_stride, k, Nkp * 256, v, Nkp * 256, Nk, self.f32[L + "cross_attn_image.v_proj.bias"])
            x = self._gemm_b(O, R, L + "cross_attn_image.out_proj", B, 4096, res=x_res, stride_res=res_stride)
            tb = self._ln(x, L + "norm3", B * 4096, 256, 1e-5)
            h = self._gemm_b(tb, R, L + "linear1", B, 4096, out_bf=True, act=ACT_RELU)
            x = self._gemm_b(h, 4096 * 2048, L + "linear2", B, 4096, res=x, stride_res=R)
        return self._ln(x, "memory_attention.norm", B * 4096, 256, 1e-5, bf=False).view(B, 4096, 256)

    def _memory_conditioned_batch(self, oids: List[int], t: int, raw: torch.Tensor, reverse: bool) -> torch.Tensor:
        """_memory_conditioned of every object in `oids` on frame t: (len(oids), 4096, 256) fp32, row i = what _memory_conditioned(oids[i], ...)
        returns, bit for bit.  Objects are grouped by bank signature (group_by_signature), a group is one batch of at most object_batch."""
        if not oids:
            return self._new(0, 4096, 256)
        # layer 0 up to the queries of its cross attention reads raw + 0.1 curr_pos alone: once per frame, with the per-object route's calls
        L = "memory_attention.layers.0."
        x = self._new(4096, 256)
        self._ck(self.lib.saber_k_axpy(self._p(raw), self._p(self.curr_pos), None, 0.1, 4096, 256, self._p(x), self._s()))

        def rope1(x_f32):
            out = self._new(4096, 256, dtype=torch.uint16)
            self._ck(self.lib.saber_k_rope(self._p(x_f32), 4096, 4096, 256, 64, 10000.0, None, self._p(out), self._s()))
            return out

        tb = self._ln(x, L + "norm1", 4096, 256, 1e-5)
        q = rope1(self._lin(tb, L + "self_attn.q_proj", 4096))
        k = rope1(self._lin(tb, L + "self_attn.k_proj", 4096))
        v = self._new(4096, 256, dtype=torch.uint16)
        self._gemm(tb, self.bf[L + "self_attn.v_proj.weight"], None, 4096, 256, 256, out_bf=v)
        O = self._new(4096, 256, dtype=torch.uint16)
        if self._flash_ws is None:
            self._flash_ws = self._new(64 * 8 * 64 * 258)
        self._ck(self.lib.saber_k_flash256(self._p(q), self._p(k), self._p(v), 4096, 4096, 1.0 / 16.0, self._p(self.f32[L + "self_attn.v_proj.bias"]), self._p(O),
                                           self._p(self._flash_ws), self._flash_ws.numel(), self._s()))
        x = self._lin(O, L + "self_attn.out_proj", 4096, res=x)
        tb = self._ln(x, L + "norm2", 4096, 256, 1e-5)
        self0 = {"x": x, "q": rope1(self._lin(tb, L + "cross_attn_image.q_proj", 4096))}
        sigs = [bank_signature(self.out[oid], t, reverse, self.num_maskmem, self.num_frames) for oid in oids]
        out = self._new(len(oids), 4096, 256)
        at = {oid: i for i, oid in enumerate(oids)}
        for group in group_by_signature(oids, sigs, self.object_batch):
            res = self._memory_conditioned_group(group, t, reverse, self0)
            if len(group) == len(oids):
                return res
            out[[at[oid] for oid in group]] = res
        return out

    # ------------------------------------------------------------------ tracking
    def _track(self, oid: int, t: int, reverse: bool) -> dict:
        raw = self._frame(t, reverse)
        cond = self._memory_conditioned(oid, t, raw, reverse)
        low, obj_v, ptr = self._sam_heads(cond, None, multimask=True, slot=self._slot(t))
        mfm = self._resize(low, 256, 256, 1024, 1024, antialias=0, post=1, a=20.0, c=-10.0)       # sigmoid(high-res logits) * 20 - 10
        mem = self._encode_memory(raw, mfm, obj_v > 0)
        return {"pred_masks": self._fill_holes(low), "obj_ptr": ptr, "obj": obj_v, "mem": mem}      # filled after the memory encoder, as upstream

    def _track_from(self, cond: torch.Tensor, t: int, reverse: bool) -> dict:
        """_track after the memory attention: cond = the object's memory-conditioned features (a row of _memory_conditioned_batch)"""
        raw = self._frame(t, reverse)
        low, obj_v, ptr = self._sam_heads(cond, None, multimask=True, slot=self._slot(t))
        mfm = self._resize(low, 256, 256, 1024, 1024, antialias=0, post=1, a=20.0, c=-10.0)
        mem = self._encode_memory(raw, mfm, obj_v > 0)
        return {"pred_masks": self._fill_holes(low), "obj_ptr": ptr, "obj": obj_v, "mem": mem}      # filled after the memory encoder, as upstream

    def _track_tail_batch(self, oids: List[int], conds: torch.Tensor, t: int, reverse: bool):
        """_track_from for all objects tracked on frame t: conds (len(oids),4096,256) = their memory-conditioned features, in the order of
        oids.  In chunks of at most object_batch objects: the SAM heads of every object are enqueued without a host read between them (the
        slot's embedding is overwritten in stream order; self._raw[t] is a copy of its own), ONE host wait fetches the chunk's object scores
        and IoUs, then the object pointers, the memory encoder, the hole fill run once for the chunk.  Returns ([the output of every object, as
        _track_from returns it, bit for bit], the (len(oids),256,256) stack of their pred_masks when they lie in one tensor in the order of
        oids, else None)."""
        raw = self._frame(t, reverse)
        slot = self._slot(t)
        if self._pad_point is None:
            self._pad_point = (torch.zeros(1, 2, device=self.dev), torch.full((1,), -1, dtype=torch.int32, device=self.dev))
            self._no_obj_plane = torch.full((256, 256), NO_OBJ_SCORE, device=self.dev)
        pts, lab = self._pad_point
        eng, results, stack = self.eng, [], None
        for c0 in range(0, len(oids), self.object_batch):
            B = min(self.object_batch, len(oids) - c0)
            # ---- SAM heads, enqueued only: the calls of _sam_heads, their outputs in one buffer per kind.  scores row i = [obj, -, -, -, iou x 3, -]
            low, scores, toks = self._new(B, 3, 256, 256), self._new(B, 8), self._new(B, 8, 256)
            for i in range(B):
                eng._check(self.lib.saber_set_embed_tokens(eng.h, slot, self._p(conds[c0 + i]), self._s()))
                eng._check(self.lib.saber_decode_points(eng.h, slot, self._p(pts), self._p(lab), 1, 1, None, self._p(low[i]), self._p(scores[i, 4:]),
                                                        self._p(scores[i]), self._s()))
                eng._check(self.lib.saber_get_decoder_tokens(eng.h, 1, self._p(toks[i]), self._s()))
            host = scores.cpu()              # the one synchronisation of the frame's chunk
            eng.check_finite()               # the engine's overflow counters accumulate until they are read: one check covers every decode above
            obj_v = [float(host[i, 0]) for i in range(B)]
            if self.hook is not None:
                for v in obj_v:
                    self.hook(v)
            best = [int(torch.argmax(host[i, 4:7])) for i in range(B)]
            # ---- the objects the heads predict present come first in the chunk's stacks (out_proj of the memory encoder: two groups)
            order = [i for i in range(B) if obj_v[i] > 0] + [i for i in range(B) if not obj_v[i] > 0]
            k = sum(1 for v in obj_v if v > 0)
            planes = [low[i, best[i]] if obj_v[i] > 0 else self._no_obj_plane for i in order]
            low_sel = planes[0][None] if B == 1 and k == 1 else torch.stack(planes, 0)         # one present object: its plane where it lies
            ptrs = None
            if k:
                # obj_ptr_proj on the chosen mask tokens: M = 1 per object through the GEMM's batch dimension (an M = k GEMM is another problem)
                rows = [toks[i, 3 + best[i]:4 + best[i]] for i in order[:k]]
                tok = rows[0] if k == 1 else torch.cat(rows, 0)
                h = self._gemm_b(self._to_bf(tok, k, 256), 256, "obj_ptr_proj.layers.0", k, 1, out_bf=True, act=ACT_RELU)
                h = self._gemm_b(h, 256, "obj_ptr_proj.layers.1", k, 1, out_bf=True, act=ACT_RELU)
                ptrs = self._gemm_b(h, 256, "obj_ptr_proj.layers.2", k, 1)                     # (k,1,256) fp32
            mfm = self._new(B, 1024, 1024)
            self._ck(self.lib.saber_k_resize_plane(self._p(low_sel), B, 256, 256, self._p(mfm), 1024, 1024, 0, 1, 20.0, -10.0, self._s()))
            mem = self._encode_memory_batch(raw, mfm, k)
            filled = self._fill_holes(low_sel)                                                  # after the memory encoder, as upstream
            chunk = [None] * B
            for j, i in enumerate(order):
                chunk[i] = {"pred_masks": filled[j], "obj_ptr": ptrs[j] if j < k else self.no_obj_ptr_dev, "obj": obj_v[i], "mem": mem[j]}
            results += chunk
            if B == len(oids) and order == list(range(B)):
                stack = filled
        return results, stack

    def _resize_planes(self, planes: torch.Tensor, Hv: int, Wv: int) -> torch.Tensor:
        """_resize of n stacked (256,256) planes to the video size in one launch: (n,Hv,Wv)"""
        n = planes.shape[0]
        out = self._new(n, Hv, Wv)
        self._ck(self.lib.saber_k_resize_plane(self._p(planes), n, 256, 256, self._p(out), Hv, Wv, 0, 0, 0.0, 0.0, self._s()))
        return out

    def _video_logits(self, planes: torch.Tensor, Hv: int, Wv: int) -> torch.Tensor:
        """The video-resolution logits (n,Hv,Wv) of a frame from the (n,256,256) stack of its objects' low-resolution logits, in obj_ids
        order.  With non_overlap_masks: _resize_planes and upstream's _apply_non_overlapping_constraints in one launch - at every pixel
        the first object with the highest resized logit keeps it, every other one reads min(its own, -10).  Else _resize_planes."""
        if not self.non_overlap_masks:
            return self._resize_planes(planes, Hv, Wv)
        planes = planes.contiguous()
        n = planes.shape[0]
        out = self._new(n, Hv, Wv)
        self._ck(self.lib.saber_k_resize_planes_non_overlap(self._p(planes), n, 256, 256, self._p(out), Hv, Wv, -10.0, self._s()))
        return out

    @torch.inference_mode()
    def propagate_in_video(self, start_frame_idx: int, max_frame_num_to_track: Optional[int] = None, reverse: bool = False) -> Iterator:
        """yields (frame_idx, obj_ids, video_res_mask_logits (n_obj, 1, Hv, Wv) device fp32) like upstream"""
        self._preflight()
        n = self.num_frames
        if max_frame_num_to_track is None:
            max_frame_num_to_track = n
        if reverse:
            end = max(start_frame_idx - max_frame_num_to_track, 0)
            order = range(start_frame_idx, end - 1, -1) if start_frame_idx > 0 else []
        else:
            end = min(start_frame_idx + max_frame_num_to_track, n - 1)
            order = range(start_frame_idx, end + 1)
        Hv, Wv = self.video_hw
        for t in order:
            outs = []
            conds = {}
            if self.batch_objects:
                # the memory attention of every object tracked on this frame in one set of launches (an object's output reads its own
                # memories alone, so the order of the two loops does not matter); then the rest of the frame for all of them together
                # (batch_tail), or per object in the loop below
                todo = [oid for oid in self.obj_ids if t not in self.out[oid]["cond"]]
                if todo:
                    raw = self._frame(t, reverse)
                    rows = self._memory_conditioned_batch(todo, t, raw, reverse)
                    if self.batch_tail:
                        tracked, stack = self._track_tail_batch(todo, rows, t, reverse)
                        for oid, o in zip(todo, tracked):
                            self.out[oid]["non_cond"][t] = o
                        for oid in self.obj_ids:
                            self._tracked[(oid, t)] = reverse
                        if stack is None or len(todo) != len(self.obj_ids):       # with the planes of the objects this frame is a conditioning frame of
                            stack = torch.stack([(self.out[oid]["cond"][t] if t in self.out[oid]["cond"] else self.out[oid]["non_cond"][t])["pred_masks"]
                                                 for oid in self.obj_ids], 0)
                        yield t, list(self.obj_ids), self._video_logits(stack, Hv, Wv)[:, None]
                        continue
                    conds = dict(zip(todo, rows))
            for oid in self.obj_ids:
                self._tracked[(oid, t)] = reverse
                if t in self.out[oid]["cond"]:
                    low = self.out[oid]["cond"][t]["pred_masks"]
                elif self.batch_objects:
                    o = self._track_from(conds.pop(oid), t, reverse)
                    self.out[oid]["non_cond"][t] = o
                    low = o["pred_masks"]
                else:
                    o = self._track(oid, t, reverse)
                    self.out[oid]["non_cond"][t] = o
                    low = o["pred_masks"]
                outs.append(low if self.non_overlap_masks else self._resize(low, 256, 256, Hv, Wv))
            if self.non_overlap_masks:       # the constraint reads all of the frame's objects: their planes as one stack, one launch
                yield t, list(self.obj_ids), self._video_logits(torch.stack(outs, 0), Hv, Wv)[:, None]
                continue
            yield t, list(self.obj_ids), torch.stack(outs, 0)[:, None]
