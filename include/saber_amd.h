/* saber_amd.h - C-ABI of the MI355X-native slice-wise SAM2 engine.
 *
 * Drop-in boundary for the hot path of chanzuckerberg/saber.  Each entry point
 * names the reference interface it replaces (paths relative to the reference tree):
 *
 *   saber_engine_create / set_weight / finalize
 *       <- build_sam2(cfg, ckpt, device, apply_postprocessing=True)   saber/adapters/sam2/automask.py:61-63
 *          get_sam2_checkpoint(cfg)                                   saber/pretrained_weights.py:174-202
 *   saber_prepare
 *       <- prep.prepare(image, to_rgb=True)                           saber/utils/preprocessing.py:67-80
 *          (contrast :4-18, normalize :20-37)
 *   saber_encode
 *       <- SAM2ImagePredictor.set_image(crop)  (third-party sam2; call site automask.py:66 / predictor.py:70)
 *   saber_decode_points
 *       <- SAM2ImagePredictor._predict(points, labels, mask_input, multimask_output, return_logits=True)
 *   saber_amg_generate
 *       <- FilteredSAM2MaskGenerator.generate -> SAM2AutomaticMaskGenerator.generate
 *                                                                     saber/adapters/sam2/amg.py:161-183
 *                                                                     saber/adapters/sam2/predictor.py:70
 *   saber_label_plane
 *       <- the paint loop of propagationSegmenter.slice_by_slice      saber/segmenters/propagation.py:185-186
 *   saber_separate_masks
 *       <- separate_masks(vol_masks, min_mask_area)                   saber/segmenters/utils.py:88-131
 *   saber_cc_chunk_label / saber_cc_seam_pairs / saber_cc_chunk_roots / saber_cc_chunk_finish
 *       <- the same separate_masks, one z-chunk per rank              saber/segmenters/utils.py:88-131
 *   saber_classifier_*
 *       <- Predictor(model_config, model_weights).predict / SAM2Classifier.forward
 *                                                                     saber/classifier/models/predictor.py:117-175, SAM2.py:118-197
 *   saber_smooth_labels / saber_gaussian_smoothing_3d
 *       <- fast_3d_gaussian_smoothing(volume, scale, deviceID)        saber/filters/masks.py:230-287
 *          gaussian_smoothing_3d(volume, sigma, device)               saber/filters/gaussian.py:76-138
 *   saber_smooth_labels_chunk / saber_smooth_radius / saber_label_max / saber_label_counts
 *       <- the same fast_3d_gaussian_smoothing, one z-chunk per rank  saber/filters/masks.py:230-287
 *   saber_consensus_components, saber_consensus_components_bits, saber_relabel_plane
 *       <- _consensus_based_resolution(image_shape, masks, confidences) saber/filters/masks.py:64-121
 *
 * Conventions: plain pointers and sizes only; every *_dev pointer is device memory owned by the
 * caller (e.g. a PyTorch-ROCm tensor's data_ptr()); `stream` is a hipStream_t (NULL = default
 * stream).  Every function returns 0 on success or a negative saber_status; the message is kept
 * per handle (saber_last_error).  Nothing aborts or exits.  A handle is bound to one device and
 * must not be used concurrently from two threads; different handles are independent
 * (reference threading contract: saber/utils/parallelization.py:100-135).
 */
#ifndef SABER_AMD_H
#define SABER_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct saber_engine saber_engine;

enum saber_status {
    SABER_OK = 0,
    SABER_ERR_INVALID = -1,   /* bad argument / unsupported configuration (ValueError in the reference) */
    SABER_ERR_STATE = -2,     /* call order violated (RuntimeError in the reference)                    */
    SABER_ERR_HIP = -3,       /* HIP runtime failure                                                     */
    SABER_ERR_CAPACITY = -4,  /* caller-provided output capacity exceeded                                */
    SABER_ERR_RANGE = -5      /* overflow sentinel: NaN / inf in the 16-bit arithmetic (saber_engine_check_finite) */
};

enum saber_dtype { SABER_U16 = 0, SABER_F32 = 1 };

/* cfgAMG (saber/adapters/sam2/amg.py:7-17) + the un-passed upstream defaults of
 * SAM2AutomaticMaskGenerator (mask_threshold 0.0, crop_nms_thresh 0.7, crop_overlap_ratio 512/1500). */
typedef struct saber_amg_params {
    int points_per_side;
    int points_per_batch;
    float pred_iou_thresh;
    float stability_score_thresh;
    float stability_score_offset;
    float mask_threshold;
    float box_nms_thresh;
    int crop_n_layers;
    float crop_nms_thresh;
    float crop_overlap_ratio;
    int crop_n_points_downscale_factor;
    int use_m2m;
    int multimask_output;
} saber_amg_params;

/* One AMG record: the non-array fields of the SAM-AMG dict consumed downstream
 * (saber/segmenters/base.py:128-133, saber/segmenters/utils.py:36-39,70). */
typedef struct saber_mask_meta {
    int32_t area;
    float bbox_xywh[4];
    float predicted_iou;
    float stability_score;
    float point_xy[2];
    float crop_box_xywh[4];
} saber_mask_meta;

/* trunk: "tiny" | "small" | "base" | "large" (the four sam2.1 Hiera trunks SABER can name, saber/adapters/base.py:28-33;
 * anything else is SABER_ERR_INVALID).  max_images: crops encoded per batched pass / feature slots kept resident.
 * max_prompts: prompts decoded per batched pass. */
int saber_engine_create(int device_id, const char* trunk, int max_images, int max_prompts, saber_engine** out);
void saber_engine_destroy(saber_engine* e);
/* e == NULL returns the calling thread's last create-time error. */
const char* saber_last_error(const saber_engine* e);

/* Upload one fp32 tensor under its upstream checkpoint key (e.g. "image_encoder.trunk.blocks.0.attn.qkv.weight"). */
int saber_engine_set_weight(saber_engine* e, const char* name, const float* host_data, const int64_t* shape, int ndim);
/* Check completeness, build bf16 / fused tables.  Must precede any compute call. */
int saber_engine_finalize(saber_engine* e);

/* K0.  img_dev: (H,W) uint16 or float32.  out_dev: (H,W) float32 in [0,1]. */
int saber_prepare(saber_engine* e, const void* img_dev, int dtype, int H, int W, float* out_dev, void* stream);
/* K0 for an (H,W,3) float32 array, as the reference's segment_image_2d treats RGB input (saber/adapters/sam2/predictor.py:58-59 ->
 * saber/utils/preprocessing.py:67-80): uniform_filter(size=500, reflect) over all three axes of the array (channel axis included),
 * clip +-3 sigma, ONE global min/max.  img_dev, out_dev: (H,W,3) interleaved float32.  Like saber_prepare it needs a created
 * handle only (no weights). */
int saber_prepare_rgb(saber_engine* e, const float* img_dev, int H, int W, float* out_dev, void* stream);

/* Encode n crops of one image.  img_dev: (H,W) [channels==1] or (H,W,3) float32 in [0,1];
 * crop_boxes_host: n x [x0,y0,x1,y1].  Features stay resident in slots slot0..slot0+n-1.
 * channels == -1: one grey plane that already carries the model's input normalisation; it is replicated to three channels WITHOUT the
 * ImageNet statistics (the video path's frames, saber/adapters/preprocessing.py:55-56; a stack of Z frames is a (Z*1024, 1024) image
 * whose crop boxes are the frames, so a window of frames is one batched pass). */
int saber_encode(saber_engine* e, const float* img_dev, int H, int W, int channels, const int* crop_boxes_host, int n,
                 int slot0, void* stream);
/* Copy a slot's features out as NCHW fp32: image_embed (256,64,64), feat_s0 (32,256,256), feat_s1 (64,128,128).
 * Any pointer may be NULL. */
int saber_get_features(saber_engine* e, int slot, float* image_embed_dev, float* feat_s0_dev, float* feat_s1_dev, void* stream);

/* Video (memory) path, SURVEY.md 8f-1 (reference: saber/adapters/sam2/predictor.py:232-348 driving upstream SAM2Base.track_step): a tracked
 * frame's image embedding is replaced by its memory-conditioned version before the mask decoder runs.  Tokens cross this boundary as
 * (4096, 256) fp32 in row-major (y * 64 + x) order.  get: the slot's image_embed (with no_mem_embed, as saber_encode leaves it).
 * set: overwrite it (the slot keeps its high-resolution features).  saber_get_decoder_tokens: the (n, 8, 256) output tokens of the last
 * saber_decode_points call ([obj, iou, mask0..3, point, pad]); upstream projects one mask token to the object pointer.  After a
 * saber_decode_prompts call on the 16-token route (saber_engine_set_multipoint) it returns the first 8 of each prompt's token rows
 * ([obj, iou, mask0..3, point0, point1]) of its last chunk, n <= max_prompts / 2; the mask tokens are rows 2..5 either way. */
int saber_get_embed_tokens(saber_engine* e, int slot, float* out_tokens_dev, void* stream);
int saber_set_embed_tokens(saber_engine* e, int slot, const float* tokens_dev, void* stream);
int saber_get_decoder_tokens(saber_engine* e, int n, float* out_dev, void* stream);

/* Slot state in and out of a handle (SURVEY.md 8e "Propagation path": the per-frame image encodes of one tomogram are independent and
 * shard over ranks; the tracking chain that consumes them is sequential.  Upstream keeps these per-frame features in
 * inference_state["cached_features"], sam2_video_predictor.py).  n consecutive slots from slot0, each as three fp32 device arrays in the
 * engine's token order: image_embed 4096 x 256, feat_s1 16384 x 64, feat_s0 65536 x 32.  import marks the slots as encoded; only
 * meaningful between handles built from the same model configuration and weights.  Both are plain device copies on `stream`, so a slot that
 * was exported and imported again decodes bit-identically.  The video predictor's frame-feature store (VideoPredictor(frame_store_gb=...))
 * is that cache on one handle: a window's newly encoded slots are exported to rows of three (rows, size) fp32 arrays - before
 * saber_set_embed_tokens replaces their image_embed - and a later window imports the frames it finds there instead of encoding them;
 * n consecutive slots take n consecutive rows, so the row pointers are passed with their offset. */
int saber_export_slots(saber_engine* e, int slot0, int n, float* emb_dev, float* fs1_dev, float* fs0_dev, void* stream);
int saber_import_slots(saber_engine* e, int slot0, int n, const float* emb_dev, const float* fs1_dev, const float* fs0_dev, void* stream);

/* Decode n point prompts against a slot.  pts_dev: (n,2) in model pixels (0..1024); labels_dev: (n) or NULL (=1).
 * mask_in_dev: (n,256,256) low-res logits or NULL.  multimask: 3 masks per prompt, else 1 (dynamic selection).
 * Outputs: lowres (n,M,256,256), iou (n,M), obj (n) - any may be NULL. */
int saber_decode_points(saber_engine* e, int slot, const float* pts_dev, const int* labels_dev, int n, int multimask,
                        const float* mask_in_dev, float* out_lowres_dev, float* out_iou_dev, float* out_obj_dev, void* stream);

/* The same with SEVERAL points per prompt (reference: upstream SAM2's prompt encoder as SAM2VideoPredictor.add_new_points_or_box feeds it -
 * clicks with labels 1 / 0, a box as its two corners with labels 2 / 3 in front of the clicks, label -1 = not a point; one padding point is
 * appended by the engine as upstream does when no box tensor is passed).  pts_dev: (n, points_per_prompt, 2), labels_dev: (n, points_per_prompt).
 * points_per_prompt == 1 is saber_decode_points.  More than one point makes 8 + (points_per_prompt - 1) decoder tokens per prompt: the 8-token
 * 16-bit kernels cannot carry them, so such prompts are decoded in the EXACT precision mode, or on the 16-token route of the 16-bit kernels
 * when saber_engine_set_multipoint is on (SABER_ERR_STATE otherwise). */
int saber_decode_prompts(saber_engine* e, int slot, const float* pts_dev, const int* labels_dev, int n, int points_per_prompt, int multimask,
                         const float* mask_in_dev, float* out_lowres_dev, float* out_iou_dev, float* out_obj_dev, void* stream);

/* Automatic mask generation for one image.  out_bits_dev: (max_masks, H, ceil(W/32)) uint32, bit b of word w of row y
 * = pixel (y, 32w+b).  out_meta_host: max_masks records.  Synchronises the stream before returning (a count is returned).
 * More than max_masks results: SABER_ERR_CAPACITY with *out_count = the capacity needed (nothing is written).
 * params->points_per_batch is accepted for cfgAMG parity and does NOT change any result: prompts are independent of each other in
 * SAM2's decoder, so the engine decodes them in batches of its own max_prompts (upstream batches only to bound memory). */
int saber_amg_generate(saber_engine* e, const float* img_dev, int H, int W, int channels, const saber_amg_params* params,
                       uint32_t* out_bits_dev, int max_masks, saber_mask_meta* out_meta_host, int* out_count, void* stream);

/* SAM2AutomaticMaskGenerator.postprocess_small_regions (upstream's min_mask_region_area > 0; there a host loop over OpenCV calls) on the final
 * masks of one image, on the device.  bits_in_dev: the (n,H,W32) rows saber_amg_generate returned, meta_host: their n records (in / out).
 *   1. every mask loses its 8-connected background components (holes) with fewer than min_area pixels, then - on that result - its
 *      8-connected foreground components (islands) with fewer than min_area pixels; if all islands are below min_area the largest stays
 *      (saber_k_mask_small_regions in include/saber_amd_kernels.h has the details and the one deviation from OpenCV's tie-break);
 *   2. a mask in which either pass met such a component is "changed" and scores 0, an untouched one 1; boxes are the tight boxes of the
 *      new masks ([x0, y0, x1, y1] with inclusive maxima as floats, [0, 0, 0, 0] when empty);
 *   3. greedy box NMS as torchvision.ops.nms: stable descending score order, fp32 IoU with area = (x2 - x1) (y2 - y1), suppressed when
 *      IoU > nms_thresh (upstream passes max(box_nms_thresh, crop_nms_thresh));
 *   4. the survivors in NMS order (untouched masks in their order, then changed masks in theirs) -> bits_out_dev rows 0 .. *out_count - 1
 *      and meta_host[0 .. *out_count): a surviving untouched mask keeps its record byte for byte, a changed one gets area = its new pixel
 *      count and bbox_xywh = [x0, y0, x1 - x0, y1 - y0]; predicted_iou, stability_score, point_xy and crop_box_xywh are never modified.
 * bits_out_dev: room for n rows, must not overlap bits_in_dev (which is left as it is).  Only a created handle is needed (no weights).
 * The label workspace on the handle is bounded (at most 128 MiB, at least one mask: the masks are run in chunks); the cleaned rows of the
 * call are staged in packed form.  n <= 12288 (the device NMS), H * W < 2^31, min_area >= 1; n = 0 succeeds with *out_count = 0.
 * One host synchronisation, which returns the count, the keep list and the per-mask results. */
int saber_amg_postprocess_small_regions(saber_engine* e, const uint32_t* bits_in_dev, int n, int H, int W, saber_mask_meta* meta_host, int min_area,
                                        float nms_thresh, uint32_t* bits_out_dev, int* out_count, void* stream);

/* Weight format of the Hiera stage-2 / stage-3 block GEMMs (qkv, proj, fc1, fc2: 94 % of the encoder's weights), to be chosen before
 * saber_engine_finalize.  SABER_WEIGHTS_FP8_E4M3 (BASELINE configs[4], "fp8 weights"): every output row is quantised to OCP e4m3fn with
 * one power-of-two scale per row (round to nearest even, saturating at 448).  The MFMA operands stay bf16 (activations are bf16, and the
 * quantised value times its scale is exact in bf16), accumulation fp32: this is the numerics of an fp8-weight checkpoint, not an
 * fp8-operand kernel.
 * SABER_WEIGHTS_MXFP8 (BASELINE configs[4], "fp8 weights on CDNA4 fp8 MFMA"; Hiera-L): qkv of the blocks that keep their width and both MLP
 * layers of every stage-2 / stage-3 block are stored in the OCP MX format (e4m3fn elements, one e8m0 power-of-two scale per 32
 * K-elements: the smallest with amax <= 448 * scale) and RUN on v_mfma_scale_f32_16x16x128_f8f6f4 (csrc/gemm_fp8.hip, twice the bf16
 * MFMA rate): their activation operands are quantised to the same format where they are produced (LayerNorm -> MX, GELU epilogue ->
 * MX), accumulation and the residual stream stay fp32, attention and attn.proj stay bf16.
 * Both are narrower than the reference's precision: never the default; their price against fp32 is reported by tests/test_gpu_fp8.py. */
#define SABER_WEIGHTS_BF16 0
#define SABER_WEIGHTS_FP8_E4M3 1
#define SABER_WEIGHTS_MXFP8 2
int saber_engine_set_weight_format(saber_engine* e, int format);

/* Arithmetic precision of the model (encoder + prompt / mask decoder; everything around them is fp32 or integer in either mode).
 * SABER_PRECISION_BF16 (default, the production path): bf16 MFMA operands, fp32 accumulation, fp32 residual stream and statistics -
 *   3-8e-3 rel-RMS from the reference's fp32 arithmetic after 48 Hiera blocks.
 * SABER_PRECISION_EXACT: every operand, stored activation and statistic in fp32 (GEMMs on the fp32-input MFMA, exact-erf GELU, the mask
 *   decoder as the unfolded composition upstream executes): the reference's own precision (saber/utils/io.py:127-132 runs fp32, autocast
 *   commented out), ~1e-6 from the fp32 CPU oracle; eight to nine times slower (1.2 s per cfgAMG-default slice) - a verification mode, never the default.
 * SABER_PRECISION_FP16 (round 4): the production kernels compiled for IEEE half operands (v_mfma_f32_16x16x32_f16: the bf16 forms' rate)
 *   - 10 mantissa bits on every GEMM / attention operand with fp32 accumulation, i.e. the operand width of the TF32 arithmetic the
 *   reference enables on its GPUs (saber/utils/io.py:127-130).  Same kernels, schedules, token order, workspaces and C-ABI as bf16; weights
 *   and stored activations are fp16.  What fp16 gives up is RANGE (largest finite value 65 504): saber_engine_finalize fails loudly when a
 *   weight, or a LayerNorm output bound |gamma| sqrt(C) + |beta|, cannot be represented, and at RUN time the overflow sentinel below
 *   (saber_engine_check_finite; built into saber_amg_generate) turns an activation that left the range into SABER_ERR_RANGE instead of
 *   NaN masks.  Conversions do NOT saturate: a clamped activation would be a silently wrong result.  The choice is made ONCE, before
 *   saber_engine_finalize (the weights are converted there); a handle finalized in one 16-bit type cannot be switched to the other.
 *   Not available together with the fp8 weight formats.
 * Call it with EXACT once BEFORE saber_engine_finalize (the fp32 weight copies are kept only then: +0.9 GB for Hiera-L); afterwards the
 * mode can be switched back and forth between EXACT and the handle's 16-bit type between calls on the same handle (EXACT then FP16 before
 * finalize makes a handle with both).  hipGraph replay is bypassed in exact mode. */
#define SABER_PRECISION_BF16 0
#define SABER_PRECISION_EXACT 1
#define SABER_PRECISION_FP16 2
int saber_engine_set_precision(saber_engine* e, int precision);

/* Overflow sentinel of the 16-bit modes (round 5).  A stored fp16 activation beyond 65 504 is an inf from there on: fp32
 * accumulators, the fp32 residual stream and every LayerNorm / softmax statistic carry it (as inf or NaN) into (a) the three feature maps of
 * the encoder pass, (b) the decoder batch's predicted IoUs / hypernetwork outputs and (c) the low-res logits.  The engine counts non-finite
 * values there on the device, on the caller's stream: one HBM-bound scan of the feature maps per encoder pass (16 MB per crop), two tiny
 * scans per decoder batch (the one over the hypernetwork outputs inside the kernel that packs them for dec_upscale), one fma per stored
 * pixel inside dec_upscale.  saber_amg_generate reads the counters with the records at its one
 * synchronisation and returns SABER_ERR_RANGE (nothing of that call's output may be used).  After saber_encode / saber_decode_points /
 * saber_decode_prompts (asynchronous, no synchronisation inside) call saber_engine_check_finite where the host synchronises anyway: it
 * waits for `stream`, returns SABER_ERR_RANGE with a message naming the stage when any counter is non-zero, and clears the counters.
 * bf16 handles run the same checks (their range is fp32's: a hit means NaN / inf in the input or the weights); the exact mode does not. */
int saber_engine_check_finite(saber_engine* e, void* stream);

/* hipGraph replay of saber_amg_generate's launch sequences (BASELINE configs[4]: "hipGraph-captured per-slice encode+decode"): the batched
 * encoder pass and each decoder batch are run eagerly the first time their shapes are seen on a handle, captured the second time and
 * replayed from then on (needs a non-default stream; on by default, SABER_AMD_GRAPHS=0 or saber_engine_set_graphs(e, 0) turns it off).
 * saber_engine_graph_stats: sequences captured / replayed so far on this handle. */
int saber_engine_set_graphs(saber_engine* e, int enable);
/* Co-residency experiment (round 4): the batched encoder passes of saber_amg_generate run on `stream` instead of the
 * call's own stream (fenced by events on both sides: results are identical); NULL restores the default.  With CU-masked streams
 * (saber_k_stream_create_cu_range) one handle's MFMA-bound encoder and another handle's HBM-bound decoder can be given disjoint sets of CUs. */
int saber_engine_set_encoder_stream(saber_engine* e, void* stream);
int saber_engine_graph_stats(const saber_engine* e, int* captures, int* replays);

/* Host synchronisations (hipStreamSynchronize) the last saber_amg_generate call on this handle needed: 2 per group of crops decoded
 * together + 1 at the end (7 for cfgAMG's default 1 + 4 + 16 crop pyramid), more only when a scratch buffer had to grow. */
int saber_amg_last_syncs(const saber_engine* e);
/* Where the generator's post-processing runs: 1 (default) = on the device - IoU / stability / crop-edge filters, the
 * per-crop box NMS, the cross-crop NMS and the compaction of the survivors are kernels on the caller's stream and a slice costs ONE host
 * synchronisation; 0 = the host restatement of round 1-2 (3 synchronisations).  Identical masks, order and records either way
 * (tests/test_gpu_graphs.py); generators with more than 12 288 candidates per image use the host path. */
int saber_engine_set_device_amg(saber_engine* e, int enable);
/* IoU pruning of the m2m pass (on by default; results are identical either way): a refined candidate reports its mask 0's IoU prediction or
 * the best of the other three (dynamic multimask selection, upstream sam2 MaskDecoder._dynamic_multimask_via_stability); when all four
 * predictions are <= params->pred_iou_thresh it cannot pass the `predicted_iou > pred_iou_thresh` filter of the mask generator
 * (upstream automatic_mask_generator._process_batch), so its masks are neither upscaled nor read.  saber_amg_last_pruning: how many of the
 * last saber_amg_generate call's m2m candidates were skipped. */
int saber_engine_set_iou_pruning(saber_engine* e, int enable);
/* The predictor half of upstream's min_mask_region_area (off by default; callable at any time after create; 0 / 0 restores the default):
 * SAM2AutomaticMaskGenerator(min_mask_region_area=A) builds SAM2ImagePredictor(max_hole_area=A, max_sprinkle_area=A), whose every prediction
 * cleans its 256 x 256 logits BEFORE they are resized, thresholded and scored (saber_k_clean_lowres in include/saber_amd_kernels.h has the
 * semantics).  With either area > 0, saber_amg_generate cleans - with params->mask_threshold - the planes its full-resolution masks are made
 * from, for the candidates that pass the predicted-IoU filter: the planes of the m2m pass with use_m2m (the first-pass planes feed the mask
 * prompt untouched), the first-pass planes without.  One launch per group of crops, outside the captured decode sequences; stability scores,
 * boxes and every later filter see the cleaned planes.  Areas 0..65535.  saber_decode_points / saber_decode_prompts and the video path are not
 * affected: they return upstream's uncleaned low-resolution logits. */
int saber_engine_set_lowres_cleanup(saber_engine* e, int max_hole_area, int max_sprinkle_area);
/* Prompts of 2..9 points (saber_decode_prompts) on the handle's 16-bit kernels (off by default; callable at any time after create): every
 * prompt carries 16 decoder token rows, rows 7 + points .. 15 are padding that no attention sees, and a call is run in chunks of
 * max_prompts / 2 prompts in the workspaces of max_prompts 8-token prompts (no extra memory).  0: such prompts need the EXACT precision mode
 * (SABER_ERR_STATE otherwise).  One point per prompt stays on the 8-token kernels, bit for bit; the EXACT mode ignores the switch.
 * SABER_ERR_INVALID when enabling it on a handle with max_prompts < 2. */
int saber_engine_set_multipoint(saber_engine* e, int enable);
int saber_amg_last_pruning(const saber_engine* e, int64_t* pruned, int64_t* m2m_candidates);

/* plane[y][x] = (position in order_host)+1 of the LAST mask covering the pixel, 0 if none. */
int saber_label_plane(saber_engine* e, const uint32_t* bits_dev, const int* order_host, int n, int H, int W,
                      uint16_t* plane_dev, void* stream);

/* Sliding-window masks in full-frame form (csrc/windows.hip; records and outputs: saber_amd_kernels.h, saber_k_place_window_masks /
 * saber_k_window_label_stack).  src_dev: src_words 32-bit words on the device; table_host: n records on the HOST, checked before anything
 * is launched: h, w >= 1; 0 <= y0, y0 + h <= H; 0 <= x0, x0 + w <= W; 0 <= src_word, src_word + h * ceil(w / 32) <= src_words; also
 * H W < 2^31, elem_bytes in {1, 2, 4}, 0 <= first, 0 <= count, first + count <= n and first + count <= 255 (1 byte) / 65535 (2 bytes).
 * A violation is SABER_ERR_INVALID with a message that names the record; nothing is launched and the output is untouched.  n == 0 /
 * count == 0 succeed without a launch.  The table is uploaded on `stream`; one launch, accounted under the profile class of
 * saber_label_plane; no host synchronisation.  The uploaded table lives in one buffer of the handle (it doubles when it is outgrown; an
 * outgrown buffer is released with the handle), so the calls of one handle must be issued on one stream at a time, as those of
 * saber_label_plane. */
struct saber_window_mask;
int saber_place_window_masks(saber_engine* e, const uint32_t* src_dev, int64_t src_words, const struct saber_window_mask* table_host, int n, int H,
                             int W, uint32_t* out_dev, void* stream);
int saber_window_label_stack(saber_engine* e, const uint32_t* src_dev, int64_t src_words, const struct saber_window_mask* table_host, int n, int first,
                             int count, int H, int W, int elem_bytes, void* out_dev, void* stream);

/* out_inter_dev[i*n+j] = |mask_i AND mask_j| in pixels for the n bit-packed masks: the integer counts behind
 * remove_duplicate_masks' IoU (saber/segmenters/utils.py:21-29); IoU = inter / (area_i + area_j - inter). */
int saber_mask_pair_intersections(saber_engine* e, const uint32_t* bits_dev, int n, int H, int W, int32_t* out_inter_dev, void* stream);

/* 3-D connected components of the stitched label volume (replaces saber.segmenters.utils.separate_masks,
 * saber/segmenters/utils.py:88-131, the last step of propagationSegmenter.slice_by_slice, propagation.py:189): foreground =
 * plane value != 0, 26-connectivity, components below min_mask_area * 10 voxels dropped (utils.py:113-119), survivors numbered
 * 1..K in scipy.ndimage.label's order.  planes_dev: (Z,H,W) uint16, out_dev: (Z,H,W) uint32, both on the engine's device;
 * Z*H*W < 2^31.  Synchronises the stream (the label count is returned). */
int saber_separate_masks(saber_engine* e, const uint16_t* planes_dev, int Z, int H, int W, int min_mask_area, uint32_t* out_dev,
                         int* out_n_labels, void* stream);

/* ---- the same stitch with the volume cut into consecutive z-chunks (one per rank, or one after the other on one device), csrc/cc3d.hip;
 * the host side is saber_amd/segmenters/stitch.py.  Only a created handle is needed.  A chunk's roots are chunk-local voxel indices
 * (a component's first voxel in C-order scan of the chunk); root + z0*H*W is the voxel's index in the whole volume, which must stay
 * below 2^31 - 1 as for saber_separate_masks.
 *
 * saber_cc_chunk_label: the labelling of saber_separate_masks on one chunk, into caller-owned buffers.  planes_dev: (Z,H,W) uint16;
 * lab_dev, sizes_dev: (Z,H,W) uint32.  On return (enqueued, no synchronisation) lab[v] = root of v or 0xffffffff for background, and
 * sizes[root] = voxels of the root's component inside the chunk (0 at every other index). */
int saber_cc_chunk_label(saber_engine* e, const uint16_t* planes_dev, int Z, int H, int W, uint32_t* lab_dev, uint32_t* sizes_dev, void* stream);
/* saber_cc_seam_pairs: what touches across the seam between a chunk's last plane (a) and the next chunk's first plane (b).
 * a_roots_dev, b_roots_dev: (H,W) uint32 planes of `lab`; a_offset / b_offset (z0*H*W of either chunk) are added to the roots.
 * pairs_dev: capacity x 2 uint32, receives rows (root in a, root in b) for every foreground pixel of a and every foreground pixel of b within
 * |dy| <= 1, |dx| <= 1, under the merge rule of the labelling (per row the centre neighbour if it is foreground, else the two diagonals).
 * The rows come in no particular order and may repeat; as a set they do not depend on the order of execution.  *out_count = rows found.
 * When that exceeds capacity nothing past capacity is written and the call returns SABER_ERR_CAPACITY with *out_count set: call again with
 * room for all.  Synchronises the stream. */
int saber_cc_seam_pairs(saber_engine* e, const uint32_t* a_roots_dev, const uint32_t* b_roots_dev, int H, int W, uint32_t a_offset, uint32_t b_offset,
                        uint32_t* pairs_dev, int capacity, int* out_count, void* stream);
/* saber_cc_chunk_roots: the chunk's roots with at least max(min_voxels, 1) voxels, except those in exclude_host (the roots that face a
 * seam: their component may continue in another chunk), ascending, into roots_out_host.  sizes[root] is cleared for the excluded and the
 * smaller ones (id 0 until saber_cc_chunk_finish says otherwise).  *out_count = roots found; beyond capacity SABER_ERR_CAPACITY with
 * *out_count set, and the call may be repeated.  Synchronises the stream. */
int saber_cc_chunk_roots(saber_engine* e, const uint32_t* lab_dev, uint32_t* sizes_dev, int Z, int H, int W, uint32_t min_voxels,
                         const uint32_t* exclude_host, int n_exclude, uint32_t* roots_out_host, int capacity, int* out_count, void* stream);
/* saber_cc_chunk_finish: sizes[roots_host[i]] = ids_host[i] for the k listed roots (each must be a root of `lab`), then
 * sizes[v] = sizes[root of v], 0 for background: sizes_dev then holds the chunk's (Z,H,W) uint32 labels.  To be called after
 * saber_cc_chunk_roots, with an id for every root that is to survive.  Synchronises the stream. */
int saber_cc_chunk_finish(saber_engine* e, const uint32_t* lab_dev, uint32_t* sizes_dev, int Z, int H, int W, const uint32_t* roots_host,
                          const uint32_t* ids_host, int k, void* stream);

/* Per-label adaptive 3-D Gaussian smoothing of a label volume (replaces saber.filters.masks.fast_3d_gaussian_smoothing,
 * saber/filters/masks.py:230-287; applied to the segmenter's output by segment_tomogram_core, saber/entry_points/inference_core.py:68-74
 * with scale = 0.05).  For each label value v != 0, ascending: sigma = scale * 2 (3 |vol == v| / 4 pi)^(1/3) (masks.py:289-309), separable
 * zero-padded Gaussian of int(6 sigma + 1) (made odd) taps along x, y, z in fp32 (gaussian.py:97-131), out[field > 0.5] = (uint8) v,
 * later labels overwriting earlier ones.  labels_dev: (Z,H,W) of elem_bytes 1, 2 or 4 (unsigned), values <= 2^22; out_dev: (Z,H,W)
 * uint8 (label values wrap modulo 256 exactly as the reference's uint8 result array does).  *out_n_labels = labels found.
 * Only a created handle is needed (no weights / finalize).  Synchronises the stream (per-label statistics come back to the host). */
int saber_smooth_labels(saber_engine* e, const void* labels_dev, int elem_bytes, int Z, int H, int W, double scale, uint8_t* out_dev,
                        int* out_n_labels, void* stream);

/* saber_smooth_labels for one z-chunk of a volume that is spread over several ranks (saber_amd/segmenters/smooth.py): the result on the
 * chunk's own planes, bit for bit what saber_smooth_labels gives there on the whole volume.  Three separate buffers, each (planes,H,W)
 * of elem_bytes: own_dev the chunk's planes [z0, z1), lo_dev the lo_planes planes [z0 - lo_planes, z0) below it, hi_dev the hi_planes
 * planes [z1, z1 + hi_planes) above it (a buffer of 0 planes may be NULL).  ids_host / counts_host: n_ids label values, ascending, with
 * their voxel counts in the WHOLE volume - sigma, radius and taps come from these counts, bounding boxes from the three buffers.  Every
 * label value found in the buffers must be listed.  A halo must hold at least the largest radius of the table (saber_smooth_radius)
 * unless it ends at the volume's end (lo_is_volume_end: plane z0 - lo_planes is plane 0; hi_is_volume_end: the volume ends at
 * z1 + hi_planes).  A label is convolved on the planes [z0 - r, z1 + r) only and skipped when its voxels there all lie on one side of
 * the own planes.  out_dev: (own_planes,H,W) uint8; *out_n_labels = labels convolved.  Workspace: 4 B per OWN voxel + the fp32 boxes.
 * SABER_ERR_INVALID ("smooth_labels_chunk: ..."): a label missing from the table, a short halo, label values above 2^22, a radius above
 * 284, 2^31 - 1 voxels or more over the three buffers.  Synchronises the stream. */
int saber_smooth_labels_chunk(saber_engine* e, const void* lo_dev, int lo_planes, const void* own_dev, int own_planes, const void* hi_dev,
                              int hi_planes, int lo_is_volume_end, int hi_is_volume_end, int elem_bytes, int H, int W,
                              const uint32_t* ids_host, const int64_t* counts_host, int n_ids, double scale, uint8_t* out_dev,
                              int* out_n_labels, void* stream);

/* The tap radius saber_smooth_labels / saber_smooth_labels_chunk use for a label of `count` voxels at `scale` (host arithmetic only, the
 * function the drivers themselves call): what a caller sizes the halos of saber_smooth_labels_chunk with. */
int saber_smooth_radius(int64_t count, double scale, int* out_radius);

/* The counts saber_smooth_labels_chunk's table is summed from.  saber_label_max: *out_max = the largest value of n label elements.
 * saber_label_counts: counts_dev[v] = voxels of label value v in the (Z,H,W) volume for 0 < v < n_counts, counts_dev[0] = 0 (the
 * background is not counted); int64; every value of the volume must be below n_counts.  elem_bytes 1, 2 or 4 (unsigned).  Both synchronise the stream. */
int saber_label_max(saber_engine* e, const void* labels_dev, int elem_bytes, int64_t n, uint32_t* out_max, void* stream);
int saber_label_counts(saber_engine* e, const void* labels_dev, int elem_bytes, int Z, int H, int W, int n_counts, int64_t* counts_dev,
                       void* stream);

/* The separable filter itself on one 0/1 mask with a given sigma (saber/filters/gaussian.py:76-138): mask_dev (Z,H,W) uint8,
 * out_dev (Z,H,W) float32. */
int saber_gaussian_smoothing_3d(saber_engine* e, const uint8_t* mask_dev, int Z, int H, int W, double sigma, float* out_dev, void* stream);

/* ---- organelle / membrane refinement (saber/analysis/refine_membranes.py), csrc/morph3d.hip.  Only a created handle is needed. ----
 * Binary dilation (op 0), erosion (op 1) or opening (op 2: erosion, then dilation) of a 0/1 volume by the ball of `radius` 1..16 with
 * a zero border: what _torch_dilation_3d / _torch_erosion_3d / _morphological_opening_gpu (refine_membranes.py:274-333) compute with a
 * dense conv3d of the _create_ball_kernel structuring element (:100-117, dist^2 <= radius^2), and what the scipy.ndimage.binary_opening
 * route (:309-319) computes on the CPU.  mask_dev, out_dev: (Z,H,W) uint8 on the engine's device, any non-zero voxel is set, the result
 * is 0/1.  Runs on bit-packed rows; synchronises the stream. */
int saber_morph_ball_3d(saber_engine* e, const uint8_t* mask_dev, int Z, int H, int W, int radius, int op, uint8_t* out_dev, void* stream);

/* 6-connected components (scipy.ndimage.label's default structure) of the non-zero voxels of a (Z,H,W) uint8 volume.  mode 0: components
 * with fewer than min_size voxels are zeroed (_remove_small_objects, refine_membranes.py:136-159; _remove_small_membrane_components,
 * :201-224); mode 1: only the largest component stays, the first in raster order on ties (_get_largest_component, :226-249: argmax over
 * scipy's label order).  out_dev keeps the input's values on the surviving voxels and may be the input itself.  *out_n_components =
 * components kept (mode 0) or found (mode 1).  Synchronises the stream. */
int saber_components6_3d(saber_engine* e, const uint8_t* mask_dev, int Z, int H, int W, int mode, int min_size, uint8_t* out_dev,
                         int* out_n_components, void* stream);

/* FilteringConfig (refine_membranes.py:54-63) as the device pipeline needs it.  ball_size is a RADIUS (1..16).  min_roi_size =
 * float32(min_roi_relative_size * shape), computed by the caller with the arithmetic of _get_organelle_roi (:261-266): the size test
 * `extent < min_roi_size` is a float32 comparison and is not re-derived here. */
typedef struct saber_refine_params {
    int ball_size, min_membrane_area, edge_trim_z, edge_trim_xy, keep_surface_membranes;
    float min_roi_size[3];
} saber_refine_params;

/* OrganelleMembraneFilter.run (refine_membranes.py:445-547) with _process_organelle_batch (:335-443) on the device.  org_dev: (Z,H,W)
 * organelle labels of elem_bytes 1, 2 or 4 (unsigned), values <= 2^22; mem_dev: (Z,H,W) uint8 membrane segmentation (non-zero = membrane).
 * Writes the two FLATTENED label maps, convert_to_3d_labels (:549-573) of the reference's 4-D stacks: organelle v comes out as v + 1 in
 * both maps (the reference relabels to (v + 1) * 2, :494-495, and halves at the end, :539-540), later labels overwrite earlier ones.
 * The per-pair results (label, box, packed organelle and membrane bits) stay on the handle until the next call or destroy, for
 * saber_refine_membranes_instances.  *out_n_labels_in = labels found on the planes that hold membrane (:479-480); *out_n_pairs = pairs
 * that survived (planes of the reference's stacks).  SABER_ERR_INVALID when a label exceeds 2^22 or (largest label + 1) * 2 does not fit
 * the element type (the reference wraps silently there).  Three stream synchronisations per call, whatever the number of labels. */
int saber_refine_membranes(saber_engine* e, const void* org_dev, int elem_bytes, const uint8_t* mem_dev, int Z, int H, int W,
                           const saber_refine_params* params, void* org_labels_out_dev, void* mem_labels_out_dev, int* out_n_labels_in,
                           int* out_n_pairs, void* stream);

/* Pairs [first, first + count) of the last saber_refine_membranes call as dense planes: the reference's 4-D stacks (:534-540), `count`
 * planes at a time.  org_stack_dev, mem_stack_dev: (count,Z,H,W) of elem_bytes.  SABER_ERR_INVALID for a range outside [0, n_pairs). */
int saber_refine_membranes_instances(saber_engine* e, int first, int count, int elem_bytes, void* org_stack_dev, void* mem_stack_dev,
                                     void* stream);

/* ---- organelle statistics (saber/analysis/organelle_statistics.py), csrc/labelstats.hip.  Only a created handle is needed. ----
 * What extract_organelle_statistics (organelle_statistics.py:5-79) computes per label, for every label at once: np.unique(mask) > 0
 * (:15-16), the voxel count np.sum(mask == label) (:22-25, :40) and, of skimage.measure.regionprops on that mask (:30), the centroid (:31)
 * and axis_major_length / axis_minor_length (:44-45).  The volume is read twice whatever the number of labels (which values are present;
 * their moments), where the reference makes several passes and a full-volume temporary per label.
 * labels_dev: (Z,H,W) of elem_bytes 1 (unsigned), 2 or 4, is_signed != 0 for int16 / int32; values <= 0 are background, 32-bit values
 * lie in 1..2^22, the narrow types may use their whole range.  Z, H, W <= 65535 and Z*H*W < 2^31.
 * Outputs, K rows in ascending label order, all on the engine's device, each with room for `capacity` rows:
 *   labels_out_dev   uint32[K]      the label values
 *   moments_out_dev  uint64[K][16]  n, Sz, Sy, Sx, Szz, Syy, Sxx, Szy, Szx, Syx (sums over the label's voxel coordinates), zmin, ymin,
 *                                   xmin, zmax, ymax, xmax (inclusive bounding box).  Integer accumulation: exact, the same bits every call.
 *   stats_out_dev    double[K][8]   centroid z, y, x; axis_major_length = sqrt(20 l0); axis_minor_length = sqrt(20 max(l2, 0)); l0 >= l1 >=
 *                                   l2, the eigenvalues of the covariance of the voxel coordinates (divided by n, as skimage does).  For a
 *                                   3-D region skimage's sqrt(10 (ev0 + ev1 - ev2)) and sqrt(10 (-ev0 + ev1 + ev2)) on the inertia tensor's
 *                                   eigenvalues are exactly these.  A flat label has minor length 0: the reference's equivalent-sphere
 *                                   fall-back (:52-55), reached only when rounding makes the sqrt argument negative, is not reproduced.
 * *out_n_labels = K, also when the call fails with SABER_ERR_CAPACITY because K > capacity (nothing is written then; call again with
 * room for K rows).  The 3-voxel rule (:25) is the caller's: every label > 0 gets a row.  mode 0: moments reduced per block in LDS
 * before they reach global memory; mode 1: one global update per row piece and label (the baseline mode 0 is measured against; same
 * results).  Two stream synchronisations per call, whatever K is. */
int saber_label_statistics(saber_engine* e, const void* labels_dev, int elem_bytes, int is_signed, int Z, int H, int W, int capacity, int mode,
                           uint32_t* labels_out_dev, uint64_t* moments_out_dev, double* stats_out_dev, int* out_n_labels, void* stream);

/* ---- consensus mask resolution (saber/filters/masks.py:64-121), csrc/consensus2d.hip.  Only a created handle is needed. ----
 * What _consensus_based_resolution computes from the candidate masks of the wanted class, without its per-mask and per-component passes
 * over the image: the overlap-averaged confidence of every pixel, the 4-connected components (scipy.ndimage.label's default 2-D
 * structure) of the union of the masks and, per component, area, bounding box and the sum of the averaged confidence.
 * masks_dev: (n,H,W) uint8 on the engine's device, non-zero = set.  select_host: k row indices into the stack (0 <= index < n, repeats
 * allowed), conf_host: their k float32 confidences; both HOST arrays, read before the call returns.  H, W >= 1, H*W < 2^31, 1 <= k <= n.
 * Arithmetic, per pixel: cm = the float32 sum of the confidences of the set masks, added one after the other in list order (the
 * reference's `confidence_map += seg * conf`), count = the number of set masks, avg = (double)cm / (double)count (0 where count = 0).
 * Outputs, on the engine's device, allocated by the caller:
 *   labels_out_dev  int32[H][W]   0 = background, components 1..K numbered in raster order of their first pixel (scipy's order)
 *   table_out_dev   saber_consensus_row[capacity], rows 0..K-1 written, row i = component i + 1
 * *out_n_components = K, also when the call fails with SABER_ERR_CAPACITY because K > capacity (labels_out_dev is complete then, the
 * table is not; call again with room for K rows - ceil(H*W / 2) rows always suffice).  Integer fields are exact and the same every call;
 * avg_sum is accumulated with fp64 atomics, one add per row run, so its last bits can differ between two calls (relative error within
 * area * 2^-53 of the exact sum either way).  SABER_ERR_INVALID (checked before anything is launched) for a limit above or a NULL
 * pointer.  One stream synchronisation per call, whatever k and K are; no (n,H,W)-sized temporary. */
typedef struct saber_consensus_row {
    int32_t area, x_min, y_min, x_max, y_max, reserved;   /* inclusive bounds; reserved = 0 */
    double avg_sum;                                        /* sum of avg over the component's pixels; score = avg_sum / area */
} saber_consensus_row;
int saber_consensus_components(saber_engine* e, const uint8_t* masks_dev, int n, int H, int W, const int* select_host, const float* conf_host,
                               int k, int capacity, int32_t* labels_out_dev, saber_consensus_row* table_out_dev, int* out_n_components,
                               void* stream);
/* The same on rows of the mask generator's bit-packed stack (saber_amg_generate): bits_dev (n_rows,H,W32) uint32, W32 = ceil(W / 32), bit b
 * of word w of a row = pixel 32w+b; select_host indexes its rows.  Same arithmetic (the float32 chain over the set masks in list order),
 * outputs, limits and capacity protocol; only the accumulation kernel reads another format, an eighth of the bytes. */
int saber_consensus_components_bits(saber_engine* e, const uint32_t* bits_dev, int n_rows, int H, int W, const int* select_host,
                                    const float* conf_host, int k, int capacity, int32_t* labels_out_dev, saber_consensus_row* table_out_dev,
                                    int* out_n_components, void* stream);
/* plane_dev[p] = lut_dev[labels_dev[p]] over an (H,W) int32 label plane (0 for a label outside [0, lut_len)): paints the components of a
 * consensus call with the values of a caller-built table, lut[0] = 0.  All three on the engine's device; no synchronisation. */
int saber_relabel_plane(saber_engine* e, const int32_t* labels_dev, int H, int W, const uint16_t* lut_dev, int lut_len, uint16_t* plane_dev,
                        void* stream);

/* ---- domain-expert classifier filter on the engine's image embeddings ----
 * Replaces saber.classifier.models.predictor.Predictor (saber/classifier/models/predictor.py:9-60 construction, :117-175 predict) with the
 * SAM2Classifier model (saber/classifier/models/SAM2.py:21-197) behind it; hook: saber2D._apply_classifier -> filters.apply_classifier
 * (saber/segmenters/base.py:159-176, saber/filters/masks.py:8-21).
 * A classifier is bound to a finalized engine handle (its Hiera encoder is the classifier's frozen backbone) and is used from the same
 * thread as that handle.  Weights: the state_dict entries of SAM2Classifier under their own names ("projection.0.weight", ...,
 * "projection.1.running_var", "projection.2.weight", ..., "classifier.4.bias"; num_batches_tracked is not needed), fp32 host arrays.
 * Eval-mode BatchNorm is folded into the convolutions at finalize. */
typedef struct saber_classifier saber_classifier;
int saber_classifier_create(saber_engine* e, int num_classes, saber_classifier** out);
void saber_classifier_destroy(saber_classifier* c);
int saber_classifier_set_weight(saber_classifier* c, const char* name, const float* host_data, const int64_t* shape, int ndim);
int saber_classifier_finalize(saber_classifier* c);
/* Predictor.predict: image_dev (H,W) float32 (the grey image handed to apply_classifier), masks_dev (n,H,W) uint8 candidate masks.
 * Per mask: whole-image z-score (monai NormalizeIntensity), crop_and_resize_adaptive (margin 1.5, 320x320, bilinear image / nearest
 * mask), masks whose resized crop holds fewer than min_area pixels are skipped (their row of probs stays 0, predictor.py:139-141,170-173),
 * SAM2 image embedding of the crop, ROI/RONI features, head, softmax.  probs_host: (n, num_classes) float32 HOST memory.
 * Synchronises the stream (bounding boxes, areas and the probabilities come back to the host). */
int saber_classifier_predict(saber_classifier* c, const float* image_dev, int H, int W, const uint8_t* masks_dev, int n, int min_area,
                             float* probs_host, void* stream);
/* saber_classifier_predict on rows rows_host[0..k) (a HOST array, 0 <= row < n_rows) of the mask generator's bit-packed stack bits_dev
 * (n_rows,H,W32) uint32, bit b of word w of a row = pixel 32w+b (bits past W in a row's last word are ignored).  Same semantics and the
 * same bits as saber_classifier_predict on the unpacked (k,H,W) stack of those rows: only the bounding-box kernel and the crop kernel's
 * nearest-neighbour mask tap read the other format.  probs_host: (k, num_classes).  No (k,H,W) uint8 stack is made. */
int saber_classifier_predict_bits(saber_classifier* c, const float* image_dev, int H, int W, const uint32_t* bits_dev, int n_rows,
                                  const int* rows_host, int k, int min_area, float* probs_host, void* stream);
/* SAM2Classifier.forward after the backbone, on the embeddings engine slots 0..k-1 hold now (saber_encode / saber_set_embed_tokens):
 * mask_crops_dev (k,320,320) uint8 -> probs_host (k, num_classes). */
int saber_classifier_head(saber_classifier* c, const uint8_t* mask_crops_dev, int k, float* probs_host, void* stream);
/* The 320x320 image crops / binarised mask crops the last saber_classifier_predict / _predict_bits call made for its first n masks (device copies). */
int saber_classifier_get_crops(saber_classifier* c, int n, float* crops_out_dev, uint8_t* masks_out_dev, void* stream);

/* Per-launch HIP-event profiling of the engine's own kernels, by kernel class (events are recorded on the
 * stream the kernels are launched on).  Class order: 0 gemm_bf16, 1 hiera_attention, 2 layernorm,
 * 3 decoder_attention, 4 elementwise, 5 image_ops, 6 mask_post, 7 decoder_t2i, 8 decoder_i2t, 9 decoder_upscale, 10 gemm_mxfp8 (the GEMMs on the
 * fp8 MFMA, weight format SABER_WEIGHTS_MXFP8 only).  flops / bytes are ALGORITHMIC. */
typedef struct saber_profile_class { int64_t launches; double ms; double flops; double bytes; } saber_profile_class;
#define SABER_PROFILE_CLASSES 11
int saber_profile_begin(saber_engine* e);
int saber_profile_end(saber_engine* e, saber_profile_class* out, int n_classes);

/* Algorithmic work counters (FLOPs per call) for roofline reporting. */
double saber_encoder_flops(const saber_engine* e);
double saber_decoder_flops_per_prompt(void);

#ifdef __cplusplus
}
#endif
#endif
