/* saber_amd_kernels.h - kernel-level C-ABI (plain device pointers, no engine handle).
 *
 * These expose the individual gfx950 kernels so that parity tests can check each one against the
 * CPU oracle in isolation, and so that an integrator can reuse e.g. the GEMM or the K0/K8 kernels.
 * Each returns 0 or -1; on -1 saber_k_last_error() holds the message (thread-local).
 * The torch ops they stand in for (executed by the third-party sam2 package under the reference
 * call site saber/adapters/sam2/predictor.py:70) are named per function; see SURVEY.md 8a.
 */
#ifndef SABER_AMD_KERNELS_H
#define SABER_AMD_KERNELS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* saber_k_last_error(void);
/* must be called once per device before the first kernel call (sets large-LDS attributes) */
int saber_k_init(int device_id);

/* nn.Linear / 1x1 conv:  C = epi(A[M,K] . W[N,K]^T + bias); A, W bf16 (uint16 storage), bias/res fp32.
 * act: 0 none, 1 GELU(erf), 2 ReLU, 3 sigmoid.  out_f32 / out_bf16 / bias / res may be NULL.
 * pool4: rows 4q..4q+3 max-pooled into row q. res_shift / res_mod: residual row = (row >> res_shift) % res_mod. */
int saber_k_gemm(const uint16_t* A, const uint16_t* W, const float* bias, const float* res, float* out_f32, uint16_t* out_bf16,
                 int M, int N, int K, int act, int act_last, int pool4, int res_shift, int res_mod, void* stream);

/* Same GEMM with explicit leading dimensions; w_kpad = 1 declares W rows zero-padded to a multiple of 64 in K (ldw >= padded K),
 * the layout the engine uploads weights in (enables the direct-to-LDS kernel for K = 144, 288). */
int saber_k_gemm_ld(const uint16_t* A, int lda, const uint16_t* W, int ldw, int w_kpad, const float* bias, const float* res, float* out_f32,
                    uint16_t* out_bf16, int M, int N, int K, int act, void* stream);

/* Residual step + the LayerNorm that follows it in one kernel (Hiera MultiScaleBlock: attn.proj + shortcut -> norm2, mlp.layers.1 +
 * residual -> norm1 of the next block):  y = A.W^T + bias + res -> out_f32 (and out_bf16 = bf16(y) if not NULL);
 * ln_out = bf16(LayerNorm(y) * ln_gamma + ln_beta).  N must be 144, 288 or 576 (the workgroup owns whole rows); W rows zero-padded
 * to a multiple of 64 in K (ldw >= padded K); res may alias out_f32 (in-place residual stream). */
int saber_k_gemm_rowln(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, const float* res, float* out_f32,
                       uint16_t* out_bf16, const float* ln_gamma, const float* ln_beta, float ln_eps, uint16_t* ln_out, int M, int N, int K,
                       void* stream);

/* The MLP of a Hiera block + residual + the LayerNorm that follows, in one kernel that keeps the hidden activation on chip:
 * h = bf16(GELU(A[M,C] . W1[4C,C]^T + b1));  y = h . W2[C,4C]^T + b2 + res -> out_f32 (and out_bf16 = bf16(y) if not NULL);
 * ln_out = bf16(LayerNorm(y) * ln_gamma + ln_beta).  Same roundings as saber_k_gemm_ld (GELU, bf16 out) followed by saber_k_gemm_rowln.
 * C must be 144; W1 / W2 rows zero-padded to a multiple of 64 in K (ldw1 >= 192, ldw2 >= 576); res may alias out_f32 and ln_out may alias A
 * (a row is read before it is written, by the wave that owns it). */
int saber_k_mlp_rowln(const uint16_t* A, int lda, const uint16_t* W1, int ldw1, const float* b1, const uint16_t* W2, int ldw2, const float* b2,
                      const float* res, float* out_f32, uint16_t* out_bf16, const float* ln_gamma, const float* ln_beta, float ln_eps,
                      uint16_t* ln_out, int M, int C, void* stream);

/* nn.LayerNorm over the last dim; fp32 in, fp32 and/or bf16 out. */
int saber_k_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* out_f32, uint16_t* out_bf16,
                      int rows, int C, int act, void* stream);

/* Hiera MultiScaleAttention core on contiguous windows (head_dim 72): qkv bf16 [tokens][3*heads*72]
 * -> out bf16 [tokens_q][heads*72]; nk keys per window, q_pool: queries max-pooled over 4 consecutive rows. */
int saber_k_hiera_attention(const uint16_t* qkv, uint16_t* out, int n_windows, int nk, int heads, int q_pool, void* stream);
/* Same for every trunk: head_dim 72 (large) | 96 (tiny, small) | 56 (base+); any nk (the 14x14 / 7x7 windows of the smaller
 * trunks are 196 / 49 keys); key_mask (optional, device): one byte per key of a window, zero-padded to a multiple of 128 bytes,
 * 0 = the key takes no part (window-padding rows in the global-attention blocks of those trunks). */
int saber_k_hiera_attention_ex(const uint16_t* qkv, uint16_t* out, int n_windows, int nk, int heads, int head_dim, int q_pool,
                               const uint8_t* key_mask, void* stream);

/* two-way-transformer attention (fp32 in, bf16 out), contiguous [B][n][heads*hd]. */
int saber_k_dec_attention(const float* q, const float* k, const float* v, uint16_t* out, int B, int nq, int nk, int heads, int hd,
                          int k_shared, void* stream);

/* K0: prep.prepare on a (H,W) slice; ws_dev: 4*H*W floats of scratch, minmax_dev: 2 uint32 */
int saber_k_prepare(const void* img, int dtype, int H, int W, float* out, float* ws_dev, uint32_t* minmax_dev, void* stream);

/* K8: upsample n low-res (256x256) logit maps to a crop, counts / bbox / bit-pack.  stats: n x 8 int32
 * (area, inter, union, x0, y0, x1, y1, pad). bits: n x H x ceil(W/32). */
int saber_k_mask_post(const float* lowres, int n, int crop_x0, int crop_y0, int crop_w, int crop_h, int H, int W, float thr,
                      float offset, uint32_t* bits, int32_t* stats, void* stream);
/* The same with the two optional device tables of the mask generator: idx (n int32) - mask i reads plane idx[i] of lowres; pass (n bytes) -
 * masks with 0 are skipped: their bits are left as they are and their stats are the initial record (area 0, box (1<<30, 1<<30, -1, -1)).
 * Either pointer may be null. */
int saber_k_mask_post_ex(const float* lowres, const int* idx, const uint8_t* pass, int n, int crop_x0, int crop_y0, int crop_w, int crop_h,
                         int H, int W, float thr, float offset, uint32_t* bits, int32_t* stats, void* stream);

/* K8 for several crops in one launch (the crops of one decoded group of the mask generator).  A crop is 8 int32: box x0, y0, x1, y1, kbase,
 * nm, and two words K8 does not read; its candidates are [kbase, kbase + nm), and every crop's kbase follows its predecessor's last candidate.
 * crops_host and crops_dev hold the same n_crops records, in host and in device memory.  lowres / idx / pass / bits / stats are those of
 * saber_k_mask_post_ex for the kbase[n_crops - 1] + nm[n_crops - 1] - kbase[0] candidates, candidate kbase[0] first.  The result is that of one
 * saber_k_mask_post_ex call per crop. */
int saber_k_mask_post_group(const float* lowres, const int* idx, const uint8_t* pass, const int32_t* crops_host, const int32_t* crops_dev, int n_crops,
                            int H, int W, float thr, float offset, uint32_t* bits, int32_t* stats, void* stream);

/* K1a: crop -> antialiased bilinear resize to res x res (ATen's tap rule) -> ImageNet normalisation.  img fp32 (H,W) for channels 1 / -1 or
 * (H,W,3) for channels 3; crops_dev: n x (x0, y0, x1, y1) int32 on the device; out [n][3][res][res].  channels -1: one grey plane that
 * already carries the model's normalisation (replicated, no statistics).  res must be a positive multiple of 16. */
int saber_k_resize_normalize(const float* img, int H, int W, int channels, const int* crops_dev, int n, float* out, int res, void* stream);
/* K1b: Hiera PatchEmbed Conv2d(3->C, k7 s4 p3) of pix [n_images][3][1024][1024] + bias + pos, rows in the engine's token order:
 * out [n_images][65536][C].  wt [tap = (c*7 + ky)*7 + kx][C], pos [65536][C] in token order.  C: 96 | 112 | 144. */
int saber_k_patch_embed(const float* pix, const float* wt, const float* bias, const float* pos, float* out, int n_images, int C, void* stream);

/* ---- SAM2 video (memory) path: the per-frame arithmetic the reference's segment_volume (saber/adapters/sam2/predictor.py:232-348) makes the
 * third-party video predictor run besides encoder and mask decoder (upstream sam2/modeling/{memory_attention,memory_encoder,sam2_base}.py).
 * Channels-last fp32 tensors [pixels][C], pixels in row-major (y, x) order. */
/* axial rotary encoding of q / k (RoPEAttention): rows < n_rot are rotated (token = row % side^2 on a side x side grid, theta 10000), the
 * rest (object-pointer tokens) copied; fp32 and/or bf16 out */
int saber_k_rope(const float* x, int64_t rows, int n_rot, int C, int side, float theta, float* out_f32, uint16_t* out_bf16, void* stream);
/* P[row][0..n) = softmax(scale * S[row][0..n)) as bf16; columns n..ld_p zeroed */
int saber_k_softmax_rows(const float* S, int64_t ld_s, int64_t rows, int n, float scale, uint16_t* P, int64_t ld_p, void* stream);
/* Conv2d(k3, s2, p1) of the memory encoder's mask down-sampler; w (Cout,Cin,3,3) */
int saber_k_conv3x3s2(const float* in, int H, int W, int Cin, const float* w, const float* b, int Cout, float* out, void* stream);
/* the same with the weights pre-arranged as (3,3,Cin,Cout) (Cout a multiple of 4): the layout the tracking loop keeps per model */
int saber_k_conv3x3s2_t(const float* in, int H, int W, int Cin, const float* wt, const float* b, int Cout, float* out, void* stream);
/* plane[y][x] = label wherever logits (Hv,Wv) > thr at the nearest source pixel of the output pixel centre; any_flag (optional, device
 * int) is OR-ed with 1 when a pixel was painted.  SAM2Adapter.segment_volume's _apply, saber/adapters/sam2/predictor.py:288-298. */
int saber_k_paint_nearest(const float* logits, int Hv, int Wv, float thr, int label, uint16_t* plane, int H, int W, int* any_flag, void* stream);
/* ---- propagated label volumes (csrc/labelvol.hip): what lies between the tracking loop and the 3-D stitch, without leaving the device */
/* All n objects of a frame in one launch, bit-identical to n saber_k_paint_nearest calls in list order: an output pixel takes labels_host[i]
 * of the LAST i whose logits (n,Hv,Wv) exceed thr at its nearest source pixel (floor((i + 0.5) * in / out) in double, clamped) and keeps its
 * value when none does.  labels_host: n HOST ints in 0..65535 (they travel as kernel arguments, 64 per launch; a longer list goes in
 * successive launches in ascending order).  any_flag (optional, device int) is OR-ed with 1 when a pixel was written.  n = 0 paints nothing. */
int saber_k_paint_nearest_stack(const float* logits, int n, int Hv, int Wv, const int* labels_host, float thr, uint16_t* plane, int H, int W,
                                int* any_flag, void* stream);
/* vol (Z,HW) uint16 in place: vol[z][i] = lut[z * L + vol[z][i]] where vol[z][i] < L, larger values pass through.  lut: (Z,L) uint16 on the
 * device, L >= 1.  HW may be odd (frames then start off the 16-byte boundary).  The presence filter of SAM2Adapter.segment_volume
 * (saber/adapters/sam2/predictor.py:340-346) is this call with an identity-or-zero table. */
int saber_k_relabel_frames(uint16_t* vol, int Z, int64_t HW, const uint16_t* lut, int L, void* stream);
/* acc[i] = max(acc[i], binarize ? (src[i] > 0) : src[i]) for i < n: np.maximum(final, masks3d > 0) / np.maximum(final, masks3d) of
 * saber/segmenters/propagation.py:97-99 and tomo.py:246 */
int saber_k_merge_max_u16(uint16_t* acc, const uint16_t* src, int64_t n, int binarize, void* stream);
/* for i < n with v = src[i], 0 < v < L and conf[v] > best[i] (strictly): final_labels[i] = cls[v], best[i] = conf[v].  cls (L) uint16 and conf (L)
 * float32 on the device, indexed by the label in src; entry 0 is never applied.  The per-mask loop of propagationSegmenter.multiclass_segment
 * (saber/segmenters/propagation.py:150-158) in one pass: every voxel of src carries one label. */
int saber_k_merge_class_conf(uint16_t* final_labels, float* best, const uint16_t* src, const uint16_t* cls, const float* conf, int L, int64_t n,
                             void* stream);
/* out (n,H,W) bytes, 1 where bit (x & 31) of bits[n][y][x >> 5] is set: the bool `segmentation` arrays of SAM2AutomaticMaskGenerator's
 * dict list (saber/adapters/sam2/automask.py:50-56 hands them to the segmenters), unpacked before the copy to the host */
int saber_k_unpack_masks(const uint32_t* bits, int n, int H, int W, uint8_t* out, void* stream);
/* Hole filling of mask logits (csrc/holefill.hip): upstream's fill_holes_in_mask_scores, which SAM2VideoPredictor applies to the 256 x 256
 * low-resolution logits after every single-frame inference when fill_hole_area > 0.  Each of the n_planes row-major H x W planes on its own:
 * background is in[v] <= 0.0f (both zeros are background, NaN and positive values are not), background components are 8-connected, and
 * out[v] = fill_value where v lies in a background component of at most max_area pixels, else out[v] = in[v] bit for bit.  out may be in.
 * workspace: device memory of the caller, 4-byte aligned, at least n_planes * H * W * 8 bytes (a uint32 label and a uint32 size per pixel);
 * a smaller one, max_area < 1, a shape below 1, a null pointer or n_planes * H * W >= 2^31 is an error (-1, saber_k_last_error) and nothing
 * is written.  Five launches on `stream`; no synchronisation and no allocation inside. */
int saber_k_fill_holes(const float* in, int n_planes, int H, int W, int max_area, float fill_value, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Small-region clean-up of bit-packed masks (csrc/smallregions.hip): upstream's remove_small_regions in both modes, as
 * SAM2AutomaticMaskGenerator.postprocess_small_regions applies it when min_mask_region_area > 0.  bits_in / bits_out: (n,H,W32) uint32 rows,
 * W32 = ceil(W / 32), bit b of word w of a row = pixel 32w+b; bits at x >= W are not pixels: they are ignored on input and zero on output.
 * Each mask on its own, over the whole H x W plane, rows never wrap and masks never touch:
 *   1. holes: every 8-connected component of the background with FEWER than min_area pixels becomes foreground (also at the image border);
 *   2. islands, on the result of 1: every 8-connected foreground component with fewer than min_area pixels is removed; when all of them
 *      are below min_area the largest stays, on a tie the one whose first pixel comes first in raster order (scipy.ndimage.label's
 *      numbering; OpenCV, which upstream uses, numbers 8-connected components by 2x2 blocks and can pick the other one on such a tie).
 * changed[i] = 1 when a component below min_area was met in either pass (also when no pixel differs: a single island below min_area stays
 * and counts as changed), else 0; area[i] = pixels of the new mask; box_xyxy[4 i ..] = its tight box with inclusive maxima, zeros for an
 * empty mask.  bits_out may be bits_in.  workspace: device memory of the caller, 256-byte aligned; saber_k_mask_small_regions_bytes(H, W)
 * bytes hold one mask (8 bytes per pixel, the packed rows and 256 bytes, each rounded up to 256) and the masks are run in passes of as many as
 * the workspace holds, so it need not grow with n.  A workspace below one mask (the message names the size), min_area < 1, n, H or W below
 * 1, a null pointer or H * W >= 2^31 is an error (-1, saber_k_last_error) and nothing is written.  13 launches per pass on `stream`; no
 * synchronisation and no allocation inside. */
int saber_k_mask_small_regions(const uint32_t* bits_in, int n, int H, int W, int min_area, uint32_t* bits_out, int32_t* changed, int32_t* area,
                               int32_t* box_xyxy, void* workspace, size_t workspace_bytes, void* stream);
size_t saber_k_mask_small_regions_bytes(int H, int W);
/* Clean-up of low-resolution mask logits, in place (csrc/lowres_cleanup.hip): upstream's SAM2Transforms.postprocess_masks, which
 * SAM2ImagePredictor(max_hole_area=h, max_sprinkle_area=s) applies to the 256 x 256 logits of every prediction before they are resized and
 * thresholded (SAM2AutomaticMaskGenerator(min_mask_region_area=A) builds its predictor with h = s = A).  Plane k of the call is the row-major
 * H x W plane at planes + (idx ? idx[k] : k) * H * W; with pass given, a plane whose pass[k] == 0 is skipped; idx and pass may be null,
 * each on its own.  No two k may name the same plane.  Per plane, on its ORIGINAL values, with t = thr:
 *   background is x <= t, foreground is x > t (IEEE: -0.0 is background at t = 0; a NaN is in neither set, joins nothing, never changes);
 *   components are 8-connected, per polarity; rows never wrap and planes never touch; no component is exempt at the border;
 *   max_hole_area > 0: every pixel of a background component of AT MOST max_hole_area pixels becomes (float)((double)t + 10.0);
 *   max_sprinkle_area > 0: every pixel of a foreground component of AT MOST max_sprinkle_area pixels becomes (float)((double)t - 10.0);
 *   every other pixel keeps its bits (only changed pixels are stored).  Both labellings are independent: a small hole inside a small
 *   sprinkle ends at t + 10 inside an island at t - 10.
 * 1 <= H * W <= 65536 (a plane's union-find lives in one workgroup's LDS: no workspace, whatever n is), 0 <= areas <= 65535.  Null planes,
 * n < 0, a shape or an area out of range: -1 with a "clean_lowres:" message (saber_k_last_error), nothing is launched.  n == 0 or both areas
 * 0: 0 without a launch.  Otherwise ONE launch of n workgroups on `stream`; no synchronisation, no allocation; two calls on equal input give
 * equal bytes. */
int saber_k_clean_lowres(float* planes, const int* idx, const uint8_t* pass, int n, int H, int W, float thr, int max_hole_area, int max_sprinkle_area,
                         void* stream);
/* Run-length form of bit-packed masks (csrc/rle.hip): upstream's uncompressed RLE, what SAM2AutomaticMaskGenerator returns with
 * output_mode="uncompressed_rle".  A mask is flattened in column-major order (pixel (y, x) has position x H + y); its `counts` alternate runs
 * of zeros and ones, start with a zeros run (0 when pixel (0,0) is set) and sum to H W.  bits: (n,H,W32) uint32 rows, W32 = ceil(W / 32), bit b
 * of word w of a row = pixel 32w+b; bits at x >= W are not pixels: ignored on input, zero on output.  H W < 2^31; counts are uint32.
 *   saber_k_rle_count    offsets[0 .. n] <- the exclusive sum of the masks' numbers of entries (offsets[n] = the total), 64-bit, on the device.
 *                        Three launches.  It leaves per-column ranks in `ws` for the encode.
 *   saber_k_rle_encode   counts[offsets[i] .. offsets[i + 1]) <- the entries of mask i.  `ws` must be what saber_k_rle_count left for the same
 *                        stack, `offsets` its output; capacity = entries `counts` holds.  One launch, no atomics: two calls give identical
 *                        bytes.  The capacity check reads offsets[n] back (8 bytes, one wait on `stream`); no entry is written beyond a
 *                        mask's range or the capacity whatever `ws` holds.
 *   saber_k_rle_decode   bits_out (n,H,W32) <- the masks of the runs counts[offsets[i] .. offsets[i + 1]).  Runs are clamped at H W and pixels
 *                        behind the last run are zero, so malformed counts never write outside bits_out.  A memset and two launches.
 * workspace: device memory of the caller, 16-byte aligned, saber_k_rle_workspace_bytes(n, H, W) bytes (8 bytes per mask column; 0 for a shape
 * that is an error).  A null pointer, n, H or W below 1, H W >= 2^31, a workspace below that size (the message names it) or a capacity below
 * offsets[n] is an error (-1, saber_k_last_error starts with "rle_count:", "rle_encode:" or "rle_decode:") and nothing is written.  No
 * allocation inside; apart from the encode's capacity check no synchronisation. */
size_t saber_k_rle_workspace_bytes(int n, int H, int W);
int saber_k_rle_count(const uint32_t* bits, int n, int H, int W, int64_t* offsets, void* ws, size_t ws_bytes, void* stream);
int saber_k_rle_encode(const uint32_t* bits, int n, int H, int W, const int64_t* offsets, uint32_t* counts, int64_t capacity, void* ws, size_t ws_bytes,
                       void* stream);
int saber_k_rle_decode(const uint32_t* counts, const int64_t* offsets, int n, int H, int W, uint32_t* bits_out, void* stream);
/* Sliding-window masks (csrc/windows.hip): the masks of saber2D.segment_image(use_sliding_window=True) (saber/segmenters/base.py:103-150) are
 * window-sized; rasterize_masks (:214-232) pastes each into a full frame and masks_to_array (saber/filters/masks.py:157-182) stacks them.
 * A record names one window-sized bit-packed mask inside a ragged buffer `src` of 32-bit words: it occupies h * ceil(w / 32) words from
 * src + src_word, row-major with row pitch ceil(w / 32), bit b of word k of a row = pixel x = 32k + b (the generator's layout), and its pixel
 * (0, 0) lies at pixel (y0, x0) of the H x W frame.  Bits at x >= w of a row's last word are not pixels: they may hold anything. */
typedef struct saber_window_mask {
    int64_t src_word;
    int32_t y0, x0, h, w;
} saber_window_mask;
/*   saber_k_place_window_masks   out (n,H,W32) uint32, W32 = ceil(W / 32): mask i in full-frame rows, zero outside its window, zero at x >= W.
 *                                Every word of out is written exactly once (no memset, no atomics): one launch, whatever n is.
 *   saber_k_window_label_stack   out (count,H,W) of elem_bytes = 1, 2 or 4 (unsigned): plane i holds first + i + 1 where mask first + i covers
 *                                the pixel and 0 elsewhere - planes first .. first + count - 1 of masks_to_array's stack.  Every element is
 *                                written exactly once: one launch.
 * table_dev: n (place) / at least first + count (stack) records ON THE DEVICE, 8-byte aligned.  The raw entries check the call's own
 * arguments only (a null pointer, a negative count, a shape below 1, H W >= 2^31, elem_bytes, first + count against the element's range:
 * -1, saber_k_last_error starts with "place_window_masks:" / "window_label_stack:", nothing is launched); the records are the caller's
 * responsibility: every window inside the frame and inside src (saber_place_window_masks / saber_window_label_stack of saber_amd.h check them
 * on the host).  n == 0 / count == 0: 0 without a launch.  No synchronisation and no allocation inside; two calls give equal bytes. */
int saber_k_place_window_masks(const uint32_t* src, const saber_window_mask* table_dev, int n, int H, int W, uint32_t* out, void* stream);
int saber_k_window_label_stack(const uint32_t* src, const saber_window_mask* table_dev, int first, int count, int H, int W, int elem_bytes, void* out,
                               void* stream);
/* depth-wise Conv2d(k7, p3) of the memory fuser's ConvNeXt blocks; w (C,1,7,7) */
int saber_k_dwconv7(const float* in, int H, int W, int C, const float* w, const float* b, float* out, void* stream);
/* the video predictor's mask_downsample: Conv2d(1, 1, k4, s4) */
/* saber_k_dwconv7 with the weights given as (7,7,C) [tap][channel] */
int saber_k_dwconv7_t(const float* in, int H, int W, int C, const float* wt, const float* b, float* out, void* stream);
/* saber_k_conv3x3s2_t / saber_k_dwconv7_t over `batch` objects that share the weights (the tracked objects of a video frame): object i reads
 * in + i * in_stride and writes out + i * out_stride (strides in elements: multiples of 4, at least one plane when batch > 1; pointers 16-byte
 * aligned).  Every object's plane is what the single entry writes for it, bit for bit; one weight load serves a block of 4 objects. */
int saber_k_conv3x3s2_t_batched(const float* in, int64_t in_stride, int H, int W, int Cin, const float* wt, const float* b, int Cout,
                                float* out, int64_t out_stride, int batch, void* stream);
int saber_k_dwconv7_t_batched(const float* in, int64_t in_stride, int H, int W, int C, const float* wt, const float* b,
                              float* out, int64_t out_stride, int batch, void* stream);
int saber_k_conv4x4s4(const float* in, int H, int W, const float* w, const float* b, float* out, void* stream);
/* F.interpolate(mode="bilinear", align_corners=False, antialias) of n planes, fused post transform: 0 none, 1 a*sigmoid(v)+c, 2 a*(v>0)+c, 3 a*v+c, 4 (v>=a) */
int saber_k_resize_plane(const float* in, int n_planes, int H, int W, float* out, int Ho, int Wo, int antialias, int post, float a, float c, void* stream);
/* saber_k_resize_plane(antialias 0, post 0) of the n_planes contiguous (H,W) planes of one video frame - its objects, in obj_ids order - with
 * upstream's non-overlapping constraint (SAM2Base non_overlap_masks: _apply_non_overlapping_constraints on the video-resolution logits) applied
 * in the same launch.  With v[i] the bits saber_k_resize_plane writes for plane i at a pixel: out[i] = v[i] for the first i that attains
 * max_i v[i] (torch.argmax), out[i] = min(v[i], suppress_max) for every other plane (torch.clamp(max=-10.0): suppress_max is -10).
 * n_planes = 1 is the plain resize, n_planes = 0 returns 0 without a launch; any number of planes is served by one launch.  A null pointer,
 * n_planes < 0, a side below 1 or an input side above 2^22 is an error (-1, saber_k_last_error) answered before any launch.  Inputs are finite.
 * out must not overlap in.  No synchronisation and no allocation inside. */
int saber_k_resize_planes_non_overlap(const float* in, int n_planes, int H, int W, float* out, int Ho, int Wo, float suppress_max, void* stream);
/* MXFP8 GEMM on the block-scaled MFMA v_mfma_scale_f32_16x16x128_f8f6f4 (row g-1): out = act(A . W^T + bias) (+ res).  Operands in the OCP MX
 * format: e4m3fn elements ([M][lda] / [N][ldw] bytes, K contiguous, zero-padded to Kp, a multiple of 128) + one e8m0 scale byte per 32
 * K-elements, stored K-step-major: S[Kp / 128][rows][4] (rows >= the operand's rows rounded up to whole tiles: a multiple of 768 for A, of 192 for W).
 * Exactly one output: out_f32 (+ res, both with leading dimension ldc; out_bf16 may be given too and receives a copy) | out_bf16 | out_mx
 * (+ out_mx_scales [N / 128][out_mx_rows][4]: the result as the next GEMM's MX operand, N % 128 == 0).  act: 0 none, 1 GELU. */
int saber_k_gemm_mx(const uint8_t* A, int64_t lda, const uint8_t* SA, int64_t sa_rows, const uint8_t* W, int64_t ldw, const uint8_t* SW, int64_t sw_rows, const float* bias,
                    const float* res, float* out_f32, uint16_t* out_bf16, uint8_t* out_mx, uint8_t* out_mx_scales, int64_t out_mx_rows, int64_t ldc, int64_t M, int N, int Kp,
                    int act, void* stream);
/* bf16 [M][C] -> MX (C % 32 == 0): per 32-element block the smallest power-of-two scale with amax <= 448 * scale, elements round to nearest even */
int saber_k_quant_mx(const uint16_t* x, int64_t ldx, int C, uint8_t* out, int64_t ldo, int Kp, uint8_t* scales, int64_t scale_rows, int64_t M, void* stream);
/* LayerNorm over C of fp32 rows, written straight as an MX operand */
int saber_k_ln_mx(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, int C, uint8_t* out, int64_t ldo, int Kp, uint8_t* scales, int64_t scale_rows,
                  int64_t M, void* stream);
/* torchvision.ops.nms as the mask generator's device path runs it (csrc/amg_device.hip: stable descending score order, suppress box IoU >
 * iou_thresh, fp32): boxes (n,4) xyxy, scores (n), n <= 12288; scratch: n * 64 bytes; keep_out (n) receives the kept indices in score order,
 * count_out their number.  One workgroup. */
int saber_k_box_nms(const float* boxes_xyxy, const float* scores, int n, float iou_thresh, void* scratch, int* keep_out, int* count_out, void* stream);
/* one-head attention of 256 channels, flash style (the memory attention of the video path, upstream MemoryAttentionLayer self / cross attention):
 * out = bf16(softmax(scale Q K^T) V + bias_v); Q [n_q][256], K, V [n_keys][256] bf16 row-major, n_q a multiple of 64; ws: scratch of at least
 * (n_q / 64) * 8 * 64 * 258 floats for the split over the keys, or NULL */
int saber_k_flash256(const uint16_t* Q, const uint16_t* K, const uint16_t* V, int n_q, int n_keys, float scale, const float* bias_v, uint16_t* out, float* ws,
                    int64_t ws_floats, void* stream);
/* one axis (0: rows, 1: columns) of scipy.ndimage.gaussian_filter(sigma, mode="mirror", truncate=4) on n planes of H x W: the anti-aliasing filter
 * skimage.transform.resize applies before it down-samples a tomogram slice to the model's 1024 px (saber/adapters/preprocessing.py:21) */
int saber_k_gauss_mirror(const float* in, float* out, int n_planes, int H, int W, int axis, double sigma, void* stream);
/* ---- slab preparation of tomoSegmenter.segment_vol (saber/segmenters/tomo.py:98-101; csrc/volprep.hip) */
/* 1-D correlation along `len` of a contiguous (outer, len, inner) array with zero ("same") padding: scipy.ndimage.correlate1d(mode="constant"),
 * the conv1d of saber.filters.gaussian.gaussian_smoothing.  out[o][l][i] = sum_k taps[k] * in[o][l + k - ks/2][i], fp32 fma chain in ascending
 * k starting from 0.  in: dtype 0 float32, 1 int16, 2 uint16, 3 uint8 (widened exactly); out: fp32, a separate buffer (in is never written).
 * taps_host: ks HOST floats, ks odd, 3..63 (15 = sigma 5 is the tuned case).  chunk_len: outputs per thread along `len` in the ks = 15
 * kernel for inner > 1 (rounded up to a multiple of 8), 0 = chosen from the shape.  minmax_dev (optional): two device floats that receive
 * min and max of everything written to out (NaNs are ignored), in the same pass. */
int saber_k_correlate1d_zero(const void* in, int dtype, float* out, int64_t outer, int64_t len, int64_t inner, const float* taps_host, int ks,
                             int chunk_len, float* minmax_dev, void* stream);
/* preprocess.normalize(rgb=False) in place: v = (v - lo) / ((hi - lo) + 1e-8f) with lo = minmax_dev[0], hi = minmax_dev[1] read on the device;
 * fp32 subtraction, addition and IEEE division, one rounding each */
int saber_k_normalize_minmax(float* v, int64_t n, const float* minmax_dev, void* stream);
/* preprocess.project_tomogram: out (H,W) = (vol[z0] + vol[z0+1] + ... + vol[z1-1]) / float(z1 - z0), fp32 sum in ascending z, then one IEEE division
 * (numpy's mean over axis 0); 0 <= z0 < z1 <= Z, an empty range is refused */
int saber_k_project_mean(const float* vol, int Z, int H, int W, int z0, int z1, float* out, void* stream);
/* out = x + alpha * g[c] * y  (x, g may be NULL) */
int saber_k_axpy(const float* x, const float* y, const float* g, float alpha, int64_t rows, int C, float* out, void* stream);
/* out = x + y[row % y_rows] as bf16 and/or fp32 (y may be NULL) */
int saber_k_add_to_bf16(const float* x, const float* y, int y_rows, uint16_t* out_bf16, float* out_f32, int64_t rows, int C, void* stream);
/* widen stored bf16 (the memory bank keeps spatial memories in bf16, as upstream does) to fp32 */
int saber_k_bf16_to_f32(const uint16_t* x, int64_t n, float* out, void* stream);
/* batched bf16 GEMM C[b] = A[b] . W[b]^T + bias with explicit leading dimensions and batch strides */
int saber_k_gemm_batched(const uint16_t* A, int lda, int64_t strideA, const uint16_t* W, int ldw, int64_t strideW, const float* bias, float* out_f32,
                         int ldcf, int64_t strideCf, uint16_t* out_bf16, int ldcb, int64_t strideCb, int M, int N, int K, int batch, void* stream);

/* ---- the memory attention of all tracked objects of a frame in one set of launches (VideoPredictor(batch_objects=True)).  Each entry gives
 * every object of the batch the bits of the single-problem entry it stands for. */
/* saber_k_flash256 for `batch` problems of one shape: object b reads Q + b * q_stride (0: the queries are shared), K + b * k_stride, V + b * v_stride
 * and writes out + b * o_stride (strides in elements, multiples of 8).  The split over the keys is the one saber_k_flash256 picks for ONE problem
 * of n_q / n_keys; ws: batch * (n_q / 64) * split * 64 * 258 floats (NULL: no split, as saber_k_flash256; non-NULL but too small: an error) */
int saber_k_flash256_batched(const uint16_t* Q, int64_t q_stride, const uint16_t* K, int64_t k_stride, const uint16_t* V, int64_t v_stride, int n_q, int n_keys,
                             int batch, float scale, const float* bias_v, uint16_t* out, int64_t o_stride, float* ws, int64_t ws_floats, void* stream);
/* saber_k_rope on `batch` stacked blocks of rows_per rows: a row is rotated when row % rows_per < n_rot, with the token of row % rows_per
 * (the keys of stacked memory banks: every bank's pointer-token rows are copied) */
int saber_k_rope_batched(const float* x, int64_t rows_per, int batch, int n_rot, int C, int side, float theta, float* out_f32, uint16_t* out_bf16, void* stream);
/* the memory banks of `batch` objects: mem_out[b] = [n_mem stored (4096, 64) 16-bit memories ..., n_ptr_rows pointer-token rows], kin_out[b] =
 * 16-bit(float(mem) + position), both [batch][Nkp][64] with Nkp = (4096 n_mem + n_ptr_rows) rounded up to 64 and the rows beyond the bank zero.
 * mem_ptrs / pos_idx: batch * n_mem HOST entries (object-major): device pointers of the memories (n_mem <= 7) and the index of each memory's
 * position table in pos_tables [n_tables][4096][64] fp32; ptr_tok (16-bit) / ptr_pos (fp32): [n_ptr_rows][64] per object at the given element
 * strides (0: shared by the batch), NULL with n_ptr_rows = 0.  What saber_k_bf16_to_f32 + saber_k_add_to_bf16 compute on a concatenated bank. */
int saber_k_membank_assemble(const void* const* mem_ptrs, const int* pos_idx, int n_mem, const float* pos_tables, int n_tables, const uint16_t* ptr_tok,
                             int64_t ptr_tok_stride, const float* ptr_pos, int64_t ptr_pos_stride, int n_ptr_rows, int batch, uint16_t* mem_out, uint16_t* kin_out,
                             void* stream);
/* saber_k_gemm_ld for `batch` problems that share W and bias: object b reads A + b * strideA (and res + b * strideRes; 0: a shared residual) and
 * writes out_f32 + b * strideCf / out_bf16 + b * strideCb, leading dimensions N.  Every object keeps its own M, so it takes the kernel - and the
 * summation order - of the single call.  Shapes for which saber_k_gemm_ld reads W packed per K-step are refused (that route has no batch). */
int saber_k_gemm_ld_batched(const uint16_t* A, int lda, int64_t strideA, const uint16_t* W, int ldw, int w_kpad, const float* bias, const float* res,
                            int64_t strideRes, float* out_f32, int64_t strideCf, uint16_t* out_bf16, int64_t strideCb, int M, int N, int K, int act, int batch,
                            void* stream);

/* engine token order helpers (DESIGN.md "token order") */
/* Folded image->token attention of the two-way transformer (reference: sam2 TwoWayAttentionBlock.cross_attn_image_to_token +
 * norm4, called from sam2/modeling/sam/transformer.py via saber/adapters/sam2/automask.py's predictor):
 * Xout[p][n] = LN(x_n + softmax_heads(x_n Kt_p^T + kscale * blockdiag_h(tk_p[h]) peq_n[h] + cb_p) VtT_p^T + bo).
 * X [P or 1][4096][256] bf16 (x_batch_stride 0 = shared); Kt [P][64][256] bf16 = the token keys folded through W_q (8 heads x 8
 * tokens, log2e/sqrt(d) folded in); the positional term (pe_n Kt^T in the plain formula) enters through peq = pe W_q^T
 * [4096][128] bf16 (model constant) and the un-folded token keys tk [P*8][128] f32; cb [P][64]; VtT [P][256][64] bf16. */
int saber_k_dec_i2t(const uint16_t* X, int64_t x_batch_stride, const uint16_t* peq, const uint16_t* Kt, const float* tk, float kscale, const float* cb,
                    const uint16_t* VtT, const float* bo, const float* gamma, const float* beta, float eps, uint16_t* Xout, int P, void* stream);

/* saber_k_dec_i2t for prompts of 16 decoder tokens (the 16-token route, saber_engine_set_multipoint): 128 score columns c = 16 h + t, the
 * softmax over the 16 tokens of each head, columns t >= nvalid (the padding tokens) get exactly zero weight.  Kt [P][128][256] bf16,
 * tk [P*16][128] f32 (un-folded token keys, positional term kscale * tk_p[16h+t][h] . peq_n[h]), cb [P][128], VtT [P][256][128] bf16. */
int saber_k_dec_i2t16(const uint16_t* X, int64_t x_batch_stride, const uint16_t* peq, const uint16_t* Kt, const float* tk, float kscale, const float* cb,
                      const uint16_t* VtT, const float* bo, const float* gamma, const float* beta, float eps, uint16_t* Xout, int P, int nvalid, void* stream);

/* Folded token->image attention (cross_attn_token_to_image / final_attn_token_to_image):
 * out[p][t] = Wv (sum_n softmax_n(Qt_p[h,t].x_n + qscale * tq_p[h,t].pek_n[h]) x_n) + bv.
 * Qt [P][64][256] bf16 (queries folded through W_k), pek = pe W_k^T [4096][128] bf16 (model constant), tq [P*8][128] f32 (un-folded
 * projected queries), part_ws [P*split*64*256] f32, ml_ws [P*split*64*2] f32, out [P][8][128] bf16. */
int saber_k_dec_t2i(const uint16_t* X, int64_t x_batch_stride, const uint16_t* pek, const uint16_t* Qt, const float* tq, float qscale, float* part_ws,
                    float* ml_ws, int P, int split, const uint16_t* Wv, const float* bv, uint16_t* out, void* stream);

/* Head of the mask decoder (reference: sam2/modeling/sam/mask_decoder.py MaskDecoder.predict_masks, everything after the two-way transformer:
 * output_upscaling with the high-resolution features + the hypernetwork product), one fused kernel (csrc/decoder_fused.hip dec_upscale_kernel):
 *   u1 = GELU(LN2d_64(ConvT_k2s2(x; w0, b0) + feat_s1));  u2 = GELU(ConvT_k2s2(u1; w3, b3) + feat_s0);  masks4[p][k][y][x] = sum_c hyper[p][k][c] u2[c][y][x]
 * (LayerNorm over the 64 channels, eps 1e-6, biased variance; exact-erf GELU evaluated by a fitted form, |error| <= 2.6e-5 absolute).
 * X [P][4096][256] 16-bit: the transformer's image tokens, row saber_k_perm_index(y, x, 2) = token (y, x) of the 64 x 64 grid.
 * w0 = output_upscaling.0.weight [256][64][2][2], b0 [64], w3 = output_upscaling.3.weight [64][32][2][2], b3 [32]: fp32 in checkpoint layout (device or
 * host pointers); they are packed by the function saber_engine_finalize packs them with and rounded to the operand type.  ln_gamma / ln_beta [64] f32.
 * fs1 [slots][16384][64], fs0 [slots][65536][32] f32: the high-resolution features channels-last, row saber_k_perm_index(y, x, 1) / (y, x, 0) of the
 * 128 / 256 grid; prompt p reads slot (p + slot_off) / slot_div (slot_div > 0, slot_off >= 0; the caller provides (P - 1 + slot_off) / slot_div + 1 slots).
 * hyper [P][4][32] f32; masks4 [P][4][256][256] f32 out, row-major pixels.
 * 16-bit roundings: X, w0, w3 as given; u1 (the B operand of the second ConvT's MFMA) and u2 (the B operand of the hypernetwork MFMA) are rounded to
 * the operand type; hyper enters as a hi + lo pair of that type (not rounded); everything else is fp32.
 * live (optional, [P] bytes): prompts whose flag is 0 are skipped, their four planes are not written.  iou4 (optional, [P][4] f32): only the planes a
 * selection can return are written - multimask: planes 1-3; single mask: plane 0 and plane 1 + (first maximum of iou4[p][1..3], the rule of
 * saber_k_mask_pick / saber_k_mask_select; a NaN never wins a comparison).  sentinel (optional): incremented when a stored logit is NaN / inf, by the
 * number of lanes of the storing waves whose sticky flag is set (> 0 = something overflowed; not a count of pixels).
 * The call packs the weights into a temporary and returns after the launch has completed (it synchronises the stream; not capturable). */
int saber_k_dec_upscale(const uint16_t* X, const float* w0, const float* b0, const float* ln_gamma, const float* ln_beta, const float* w3, const float* b3,
                        const float* fs1, const float* fs0, int slot_div, int slot_off, const float* hyper, float* masks4, int P, const uint8_t* live,
                        const float* iou4, int multimask, unsigned int* sentinel, void* stream);
/* The hypernetwork operand as dec_upscale_kernel reads it (the engine runs this once per decoded batch; saber_k_dec_upscale runs it on its fp32 hyper):
 * out [P][2][4][4][8] in the operand type (512 B per prompt) = hyper [P][4][32] f32 split into hi = round(v) (half 0) and lo = round(v - hi) (half 1);
 * element [m][fg][j] is channel 4 fg + j (j < 4) or 16 + 4 fg + (j - 4) of hyper[p][m][.], the k-slot order of the hypernetwork MFMA.  Both 16-byte aligned.
 * nonfinite_counter (optional): += the number of scanning lanes that met a NaN / inf in hyper, the count of the engine's overflow sentinel over
 * the same 128 P values (a lane scans groups of four consecutive values: one group each up to P = 8, up to eight beyond; > 0 = something overflowed). */
int saber_k_hyper_pack(const float* hyper, int P, uint16_t* out, unsigned int* nonfinite_counter, void* stream);
/* The selection among the four planes (reference: MaskDecoder.forward / _dynamic_multimask_via_stability, delta 0.05, threshold 0.98), fp32:
 * multimask: out_iou [P][3] = iou4[:, 1:], out_sel untouched.  Single mask: stability = #(plane 0 > 0.05) / #(plane 0 > -0.05) in fp32 (1 when the
 * denominator is 0); stable (>= 0.98f): plane 0, else 1 + first maximum of iou4[p][1..3]; out_iou [P] = iou4 of the chosen plane, out_sel [P]
 * (may be NULL) = its index.  live (optional): prompts with flag 0 report plane 0 and iou4[p][0] without reading their planes. */
int saber_k_mask_pick(const float* masks4, const float* iou4, int P, int multimask, float* out_iou, int* out_sel, const uint8_t* live, void* stream);
/* the same selection with the copy: out_masks [P][3][256][256] = planes 1-3 (multimask) or [P][256][256] = the chosen plane; out_iou as above */
int saber_k_mask_select(const float* masks4, const float* iou4, int P, int multimask, float* out_masks, float* out_iou, void* stream);
/* live[p] = any of iou4[p][0..3] > thr (strict): whether a single-mask candidate can pass a `predicted IoU > thr` filter at all.
 * counters (optional, 2 x uint64): [0] += prompts with flag 0, [1] += P */
int saber_k_iou_live_flags(const float* iou4, int P, float thr, uint8_t* live, unsigned long long* counters, void* stream);

/* Development (co-residency experiments, tools/cu_mask_bench.py): a HIP stream restricted to CUs first_cu .. first_cu + n_cus - 1
 * (hipExtStreamCreateWithCUMask), and its release. */
int saber_k_stream_create_cu_range(int first_cu, int n_cus, void** out_stream);
int saber_k_stream_destroy(void* stream);
/* 16-bit operand type of every kernel-level entry point called from THIS thread (thread-local): 0 = bf16 (default), 1 = IEEE fp16.  The
 * uint16_t operands and outputs of saber_k_gemm*, saber_k_layernorm, saber_k_hiera_attention*, saber_k_dec_*, saber_k_flash256, ... are
 * then fp16 bit patterns; same kernels, compiled for v_mfma_f32_16x16x32_f16.  Returns the previous setting. */
int saber_k_set_operand_type(int f16);
/* the host-side fp32 -> IEEE half (round to nearest even) conversion saber_engine_finalize applies to the weights in SABER_PRECISION_FP16
 * (host pointers; no device needed) */
void saber_k_host_f32_to_f16(const float* in, uint16_t* out, int64_t n);
/* development hook: bit flags read by experimental kernel variants (0 in production) */
void saber_k_set_debug(int flags);
/* development: device buffer (uint64 per block, wave and phase) that instrumented kernels fill with s_memtime sums; NULL = off */
void saber_k_set_stamp_buffer(void* dev);

int saber_k_perm_index(int y, int x, int stage);

/* ---- the exact-precision (fp32) kernels of saber_engine_set_precision(e, SABER_PRECISION_EXACT) (csrc/exact.hip), through the launchers the
 * engine calls: every operand, product, sum and statistic in fp32.  Device pointers, row-major with explicit leading dimensions (in floats). */
/* C[b][m][n] = epi(sum_k A'[b][m][k] W[b][n][k] + bias[b][n]) for b < batch (A + b sA, W + b sW, bias + b sBias, C + b sC), with
 * A'[m][k] = A[m][k] + A2[m % a2_mod][k] summed in fp32 when A2 is given.  epi: act (0 none, 1 GELU(erf), 2 ReLU, 3 sigmoid), then + res;
 * act_last: + res, then act.  Residual row of output row m: res_rows_per > 0: ((m / res_rows_per + res_off) / res_div) * res_stride +
 * (m % res_rows_per) * ldres; else ((m >> res_shift) % res_mod, or without the modulo when res_mod = 0) * ldres.  pool4: output row q = max over
 * rows 4q .. 4q+3, + bias (M % 4 == 0; refused with act, act_last, res or A2).  A2 and the per-slot residual need 16-byte aligned rows. */
int saber_k_xg_gemm(const float* A, int64_t lda, int64_t sA, const float* A2, int64_t lda2, int64_t a2_mod, const float* W, int64_t ldw, int64_t sW,
                    const float* bias, int64_t sBias, const float* res, int64_t ldres, int res_shift, int64_t res_mod, int64_t res_rows_per,
                    int64_t res_stride, int res_div, int res_off, float* C, int64_t ldc, int64_t sC, int M, int N, int K, int act, int act_last,
                    int pool4, int batch, void* stream);
/* out = act(LayerNorm(x) * gamma + beta) over rows of C contiguous floats (biased two-pass variance); row_valid (optional): row r is written as
 * zeros where row_valid[r % valid_mod] == 0 */
int saber_k_xg_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* out, int64_t rows, int C, int act,
                         const uint8_t* row_valid, int valid_mod, void* stream);
/* o[b][i][h*hd + d] = sum_j softmax_j(scale q_i . k_j) v_j[h*hd + d] per batch entry b and head h (row pointers base + b *_bs + i * ld);
 * hd 16, 32, 56, 72 or 96.  qpool: query i is the element-wise maximum of q rows 4i .. 4i+3; kmask (optional, nk bytes shared by every batch
 * entry): 0 = the key takes no part */
int saber_k_xg_attention(int hd, const float* q, int64_t q_bs, int ldq, const float* k, int64_t k_bs, int ldk, const float* v, int64_t v_bs, int ldv,
                         float* o, int64_t o_bs, int ldo, int nq, int nk, int batch, int heads, int qpool, const uint8_t* kmask, float scale, void* stream);
/* out[r][c] = x[r][c] + y[(ymod ? r % ymod : r)][c] */
int saber_k_xg_add(const float* x, const float* y, int64_t ymod, float* out, int64_t rows, int C, void* stream);
/* out[p][j] = act((in ? in[p][j] : 0) + tab[((p + off) / div) * stride + j] + (vec ? vec[j % C] : 0)), j < rows_per * C, p < P */
int saber_k_xg_add_slot(const float* in, const float* tab, int64_t stride, int div, int off, const float* vec, float* out, int64_t rows_per, int C,
                        int P, int act, void* stream);
/* the mask prompt's first two stages: out[p][tok][16] = GELU(LN2d(conv k2s2 4->16 (GELU(LN2d(conv k2s2 1->4 (plane))))))), tok = saber_k_perm_index
 * order of the 64 x 64 grid, eps 1e-6; plane = mask_in + q * 65536 (256 x 256), q = p, or with raw4_q0 >= 0: q = i + i / 3 + 1 for i = raw4_q0 + p;
 * clamp_abs > 0 clamps the mask to +-clamp_abs first.  w1 [4][1][2][2], b1, g1, be1 [4]; w2 [16][4][2][2], b2, g2, be2 [16] */
int saber_k_xg_mask_hidden(const float* mask_in, int P, const float* w1, const float* b1, const float* g1, const float* be1, const float* w2,
                           const float* b2, const float* g2, const float* be2, float clamp_abs, int raw4_q0, float* out, void* stream);
/* masks4[p][k][y][x] = sum_c hyper[p][k][c] up[p][saber_k_perm_index(y, x, 0)][c]; up [P][65536][32], hyper [P][4][32], masks4 [P][4][256][256] */
int saber_k_xg_mask_dot(const float* up, const float* hyper, int P, float* masks4, void* stream);

#ifdef __cplusplus
}
#endif
#endif
