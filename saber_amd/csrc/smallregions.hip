// Small-region clean-up of the mask generator's masks on the device: upstream's postprocess_small_regions (sam2
// automatic_mask_generator.py; SAM2AutomaticMaskGenerator(min_mask_region_area=...)), which runs remove_small_regions on the host with OpenCV,
// one mask at a time, and a box NMS behind it.  Input and output are the generator's own bit-packed rows: (n, H, W32) uint32, bit b of word w
// of a row = pixel 32w+b.  Per mask, with A = min_area, two DEPENDENT passes over the whole H x W plane:
//   holes    the 8-connected components of the background with fewer than A pixels become foreground (no border exception)
//   islands  of the RESULT of the holes pass, the 8-connected foreground components with fewer than A pixels are removed; when every
//            component is below A the largest stays, the one whose first pixel comes first in raster order on a tie
// changed = a component below A was met in either pass (also when no pixel differs); area and the tight box come from the new mask.
// The fifth consumer of the union-find core of ccl.h, the second batched one: a pixel is a node (as in holefill.hip, whose merge kernel is
// shared), the bit rows are expanded to labels inside the workspace and packed again by the kernels that take the decisions.
//
// Kernels of one pass over a chunk of m masks, all on the caller's stream, no synchronisation and no allocation:
//   sr_aux_init     the chunk's per-mask records
//   sr_init<bg>     one wave per row: lab <- run starts of the row's background (holes) or foreground (islands) pixels, sizes <- 0.  Bits
//                   at x >= W are never pixels: a lane past the row's end is no member of either polarity
//   ccl8_merge      rows against the row above, never across planes or row ends (holefill.hip)
//   ccl_flatten, ccl_count
//   sr_fill         holes: mid = in | (pixels of background components below A), 64 pixels per ballot; changed_h
//   sr_best         islands: per root, "a component of at least A exists" / changed_i / the largest component by (size, first pixel)
//   sr_write        islands: out = the kept components' pixels, packed; area and box of the new mask, one set of atomics per row
//   sr_finish       the chunk's records -> changed, area, box_xyxy
// Labels are min-index roots (ccl.h), so every decision is the same whatever order the merges ran in.
//
// The second half of the file is the whole step on an engine handle (saber_amg_postprocess_small_regions): clean-up in chunks, scores, box
// NMS and compaction in NMS order (amg_device.hip: launch_small_regions_nms), one host synchronisation.
#include <climits>
#include <cstdio>

#include "ccl.h"
#include "engine.h"
#include "kernels.h"

// per-mask record of a chunk, 16 words
enum { SR_CH_H = 0, SR_CH_I, SR_ANYBIG, SR_AREA, SR_X0, SR_Y0, SR_X1, SR_Y1, SR_BEST /* 2 words, 8-byte aligned */, SR_AUX_WORDS = 16 };

__global__ __launch_bounds__(256) void sr_aux_init_kernel(uint32_t* __restrict__ aux, int m) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m * SR_AUX_WORDS) return;
    const int f = i % SR_AUX_WORDS;
    aux[i] = (f == SR_X0 || f == SR_Y0) ? 0x7fffffffu : 0u;
}

// is pixel x of the row set: `words` points at the row's first word
__device__ __forceinline__ bool sr_bit(const uint32_t* __restrict__ words, int x) { return (words[x >> 5] >> (x & 31)) & 1u; }

template <bool BACKGROUND>
__global__ __launch_bounds__(256) void sr_init_kernel(const uint32_t* __restrict__ bits, uint32_t* __restrict__ lab, uint32_t* __restrict__ sizes, int W,
                                                      int W32, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // wave-uniform
    const uint32_t* words = bits + row * W32;
    const uint32_t base = (uint32_t)(row * W);                 // fewer than 2^31 pixels per chunk: indices fit 32 bits
    uint32_t carry = CCL_NONE;
    for (int x0 = 0; x0 < W; x0 += 64) {                       // wave-uniform trip count
        const int x = x0 + lane;
        const uint32_t i = base + (uint32_t)x;
        const uint32_t start = ccl_run_start(x < W && sr_bit(words, x) != BACKGROUND, lane, base + (uint32_t)x0, carry);
        if (x < W) {
            lab[i] = start;
            sizes[i] = 0u;
        }
    }
}

// the two words a wave's ballot over pixels x0 .. x0+63 of a row makes
__device__ __forceinline__ void sr_store_ballot(uint32_t* __restrict__ words, int W32, int x0, int lane, unsigned long long b) {
    const int w = x0 >> 5;
    if (lane == 0) words[w] = (uint32_t)b;
    if (lane == 32 && w + 1 < W32) words[w + 1] = (uint32_t)(b >> 32);
}

__global__ __launch_bounds__(256) void sr_fill_kernel(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ lab, const uint32_t* __restrict__ sizes,
                                                      uint32_t min_area, uint32_t* __restrict__ mid, uint32_t* __restrict__ aux, int H, int W, int W32, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // wave-uniform
    const uint32_t* words = bits + row * W32;
    const uint32_t base = (uint32_t)(row * W);
    bool any_small = false;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        bool set = false, small = false;
        if (x < W) {
            const uint32_t r = lab[base + (uint32_t)x];        // CCL_NONE: a foreground pixel
            small = r != CCL_NONE && sizes[r] < min_area;
            set = small || sr_bit(words, x);
        }
        any_small = any_small || __ballot(small) != 0ull;
        sr_store_ballot(mid + row * W32, W32, x0, lane, __ballot(set));
    }
    if (lane == 0 && any_small) atomicOr(&aux[(row / H) * SR_AUX_WORDS + SR_CH_H], 1u);
}

template <typename T> __device__ __forceinline__ T sr_peek(T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// per root of the islands pass.  The largest component: the greatest (size, ~first pixel), so of equal sizes the smaller root wins.
// A wave holds 64 consecutive pixels: where they lie in one mask (always, unless the wave straddles two planes) its roots are reduced
// with shuffles and one lane updates the mask's record - a noisy mask has thousands of roots, and they would all meet at one address.
__global__ __launch_bounds__(256) void sr_best_kernel(const uint32_t* __restrict__ lab, const uint32_t* __restrict__ sizes, uint32_t min_area,
                                                      uint32_t* aux, uint32_t plane, uint32_t n) {
    const int lane = threadIdx.x & 63;
    for (uint32_t v0 = blockIdx.x * 256u + (threadIdx.x & ~63u); v0 < n; v0 += gridDim.x * 256u) {      // wave-uniform
        const uint32_t v = v0 + (uint32_t)lane;
        const bool root = v < n && lab[v] == v;
        const uint32_t sz = root ? sizes[v] : 0u;
        const bool big = root && sz >= min_area, small = root && sz < min_area;
        unsigned long long key = small ? (((unsigned long long)sz << 32) | (unsigned long long)(~v)) : 0ull;
        const uint32_t last = min(v0 + 63u, n - 1u);
        if (v0 / plane == last / plane) {
            const bool any_big = __ballot(big) != 0ull, any_small = __ballot(small) != 0ull;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                const unsigned long long o = __shfl_xor(key, d, 64);
                key = o > key ? o : key;
            }
            if (lane == 0) {
                // most waves bring nothing new: look before the atomic (the record only ever grows, so a stale look costs an atomic, no more)
                uint32_t* a = aux + (size_t)(v0 / plane) * SR_AUX_WORDS;
                if (any_big && !sr_peek(&a[SR_ANYBIG])) atomicOr(&a[SR_ANYBIG], 1u);
                if (any_small) {
                    if (!sr_peek(&a[SR_CH_I])) atomicOr(&a[SR_CH_I], 1u);
                    unsigned long long* best = reinterpret_cast<unsigned long long*>(a + SR_BEST);
                    if (key > sr_peek(best)) atomicMax(best, key);
                }
            }
        } else if (root) {
            uint32_t* a = aux + (size_t)(v / plane) * SR_AUX_WORDS;
            if (big) atomicOr(&a[SR_ANYBIG], 1u);
            else {
                atomicOr(&a[SR_CH_I], 1u);
                atomicMax(reinterpret_cast<unsigned long long*>(a + SR_BEST), key);
            }
        }
    }
}

__global__ __launch_bounds__(256) void sr_write_kernel(const uint32_t* __restrict__ lab, const uint32_t* __restrict__ sizes,
                                                       uint32_t min_area, uint32_t* __restrict__ out, uint32_t* aux, int H, int W, int W32,
                                                       int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // wave-uniform
    const uint32_t base = (uint32_t)(row * W);
    uint32_t* a = aux + (row / H) * SR_AUX_WORDS;
    // when no component reaches min_area the largest one stays; with none at all `best` is CCL_NONE, which no pixel has as its root
    const uint32_t best = a[SR_ANYBIG] ? CCL_NONE : ~a[SR_BEST];
    int area = 0, x_lo = INT_MAX, x_hi = -1;                   // wave-uniform: every lane sees the ballots
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        bool keep = false;
        if (x < W) {
            const uint32_t r = lab[base + (uint32_t)x];
            keep = r != CCL_NONE && (sizes[r] >= min_area || r == best);
        }
        const unsigned long long b = __ballot(keep);
        sr_store_ballot(out + row * W32, W32, x0, lane, b);
        if (b) {
            area += __popcll(b);
            x_lo = min(x_lo, x0 + __ffsll((long long)b) - 1);
            x_hi = x0 + 63 - __clzll((long long)b);
        }
    }
    if (lane == 0 && area > 0) {
        const uint32_t y = (uint32_t)(row % H);
        atomicAdd(&a[SR_AREA], (uint32_t)area);
        atomicMin(&a[SR_X0], (uint32_t)x_lo);
        atomicMax(&a[SR_X1], (uint32_t)x_hi);
        atomicMin(&a[SR_Y0], y);
        atomicMax(&a[SR_Y1], y);
    }
}

__global__ __launch_bounds__(256) void sr_finish_kernel(const uint32_t* __restrict__ aux, int m, int32_t* __restrict__ changed, int32_t* __restrict__ area,
                                                        int32_t* __restrict__ box) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const uint32_t* a = aux + (size_t)i * SR_AUX_WORDS;
    const bool any = a[SR_AREA] != 0u;
    changed[i] = (a[SR_CH_H] | a[SR_CH_I]) ? 1 : 0;
    area[i] = (int32_t)a[SR_AREA];
    box[4 * i] = any ? (int32_t)a[SR_X0] : 0;                  // an empty mask: [0, 0, 0, 0]
    box[4 * i + 1] = any ? (int32_t)a[SR_Y0] : 0;
    box[4 * i + 2] = any ? (int32_t)a[SR_X1] : 0;
    box[4 * i + 3] = any ? (int32_t)a[SR_Y1] : 0;
}

namespace {
inline size_t sr_align(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

// a uint32 label and a uint32 size per pixel, the packed rows between the two passes, the mask's record
size_t small_regions_bytes_per_mask(int H, int W) {
    if (H < 1 || W < 1) return 0;
    const size_t px = (size_t)H * W, words = (size_t)H * ((W + 31) / 32);
    return sr_align(px * 8) + sr_align(words * 4) + 256;
}

const char* launch_small_regions(const uint32_t* in, int n, int H, int W, int min_area, uint32_t* out, int32_t* changed, int32_t* area, int32_t* box_xyxy,
                                 void* workspace, size_t workspace_bytes, hipStream_t s) {
    static thread_local char msg[160];
    if (n < 1 || H < 1 || W < 1) return "mask_small_regions: n, H and W must be at least 1";
    if (min_area < 1) return "mask_small_regions: min_area must be at least 1";
    if (!in || !out || !changed || !area || !box_xyxy || !workspace) return "mask_small_regions: null pointer";
    const int64_t plane = (int64_t)H * W;
    if (plane >= ((int64_t)1 << 31)) return "mask_small_regions: planes of 2^31 pixels or more are not supported";
    if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)changed | (uintptr_t)area | (uintptr_t)box_xyxy) & 3u) return "mask_small_regions: pointers must be 4-byte aligned";
    if ((uintptr_t)workspace & 255u) return "mask_small_regions: the workspace must be 256-byte aligned";
    const size_t per = small_regions_bytes_per_mask(H, W);
    if (workspace_bytes < per) {
        snprintf(msg, sizeof msg, "mask_small_regions: the workspace is too small (%zu bytes per %d x %d mask, at least one mask)", per, H, W);
        return msg;
    }
    // masks per pass: what the workspace holds, with fewer than 2^31 pixels (the labels are 32-bit indices into the chunk)
    const int W32 = (W + 31) / 32;
    const int64_t chunk = std::min<int64_t>(std::min<int64_t>((int64_t)(workspace_bytes / per), n), (((int64_t)1 << 31) - 1) / plane);
    uint32_t* lab = (uint32_t*)workspace;
    uint32_t* sizes = lab + chunk * plane;
    uint32_t* mid = (uint32_t*)((char*)workspace + sr_align((size_t)(chunk * plane) * 8));
    uint32_t* aux = (uint32_t*)((char*)mid + sr_align((size_t)chunk * H * W32 * 4));
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int m = (int)std::min<int64_t>(chunk, n - i0);
        const int64_t rows = (int64_t)m * H, px = rows * W;
        const unsigned row_blocks = (unsigned)((rows + 3) / 4), px_blocks = eng_blocks(px);
        const uint32_t* src = in + i0 * H * W32;
        uint32_t* dst = out + i0 * H * W32;
        hipLaunchKernelGGL(sr_aux_init_kernel, dim3((m * SR_AUX_WORDS + 255) / 256), dim3(256), 0, s, aux, m);
        // holes
        hipLaunchKernelGGL(sr_init_kernel<true>, dim3(row_blocks), dim3(256), 0, s, src, lab, sizes, W, W32, rows);
        if (H > 1) ccl8_merge_planes(lab, H, W, px, px_blocks, s);
        ccl_flatten(lab, px, px_blocks, s);
        ccl_count(lab, sizes, W, rows, s);
        hipLaunchKernelGGL(sr_fill_kernel, dim3(row_blocks), dim3(256), 0, s, src, (const uint32_t*)lab, (const uint32_t*)sizes, (uint32_t)min_area, mid, aux, H, W,
                           W32, rows);
        // islands of what the holes pass left
        hipLaunchKernelGGL(sr_init_kernel<false>, dim3(row_blocks), dim3(256), 0, s, (const uint32_t*)mid, lab, sizes, W, W32, rows);
        if (H > 1) ccl8_merge_planes(lab, H, W, px, px_blocks, s);
        ccl_flatten(lab, px, px_blocks, s);
        ccl_count(lab, sizes, W, rows, s);
        hipLaunchKernelGGL(sr_best_kernel, dim3(px_blocks), dim3(256), 0, s, (const uint32_t*)lab, (const uint32_t*)sizes, (uint32_t)min_area, aux, (uint32_t)plane,
                           (uint32_t)px);
        hipLaunchKernelGGL(sr_write_kernel, dim3(row_blocks), dim3(256), 0, s, (const uint32_t*)lab, (const uint32_t*)sizes,
                           (uint32_t)min_area, dst, aux, H, W, W32, rows);
        hipLaunchKernelGGL(sr_finish_kernel, dim3((m + 255) / 256), dim3(256), 0, s, (const uint32_t*)aux, m, changed + i0, area + i0, box_xyxy + 4 * i0);
    }
    return nullptr;
}

// ------------------------------------------------------------------------------------------------ the whole step on a handle
// Label workspace of the handle: as many masks as fit SR_WS_BUDGET, at least one - it does not depend on n.  The cleaned rows of all n masks
// are staged in packed form (an eighth of a byte per pixel; the NMS order is only known when every mask is done) next to 7 n + 1 result words.
#define SR_WS_BUDGET ((size_t)128 << 20)

extern "C" int saber_amg_postprocess_small_regions(saber_engine* e, const uint32_t* bits_in_dev, int n, int H, int W, saber_mask_meta* meta_host, int min_area,
                                                   float nms_thresh, uint32_t* bits_out_dev, int* out_count, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (out_count) *out_count = 0;
    const std::string who = "postprocess_small_regions: ";
    if (n < 0 || H < 1 || W < 1) return eng_fail(e, SABER_ERR_INVALID, who + "n must be at least 0, H and W at least 1");
    if (min_area < 1) return eng_fail(e, SABER_ERR_INVALID, who + "min_area must be at least 1");
    if (!out_count || (n > 0 && (!bits_in_dev || !bits_out_dev || !meta_host))) return eng_fail(e, SABER_ERR_INVALID, who + "null pointer");
    if (n == 0) return SABER_OK;
    if (n > AMG_NMS_MAX) return eng_fail(e, SABER_ERR_INVALID, who + "more masks than the device NMS holds (" + std::to_string(AMG_NMS_MAX) + ")");
    if ((int64_t)H * W >= ((int64_t)1 << 31)) return eng_fail(e, SABER_ERR_INVALID, who + "images of 2^31 pixels or more are not supported");
    const size_t words = (size_t)H * ((W + 31) / 32);
    {
        const uintptr_t a = (uintptr_t)bits_in_dev, b = (uintptr_t)bits_out_dev, len = (uintptr_t)n * words * 4;
        if (a < b + len && b < a + len) return eng_fail(e, SABER_ERR_INVALID, who + "the output rows must not overlap the input rows");
    }
    hipStream_t s = (hipStream_t)stream;
    ENG_DEVICE(e);
    const size_t per = small_regions_bytes_per_mask(H, W);
    const size_t ws_need = per * std::max<size_t>(1, std::min<size_t>((size_t)n, SR_WS_BUDGET / per));
    if (e->sr_ws_bytes < ws_need) {
        if (e->sr_ws) {
            ENG_HIP(e, hipStreamSynchronize(s));               // the old workspace may still be in use
            eng_free(e, e->sr_ws);
            e->sr_ws = nullptr;
            e->sr_ws_bytes = 0;
        }
        const int st = eng_alloc_bytes(e, &e->sr_ws, ws_need);
        if (st != SABER_OK) return st;
        e->sr_ws_bytes = ws_need;
    }
    const size_t off_res = sr_align((size_t)n * words * 4), off_cand = off_res + sr_align(((size_t)7 * n + 1) * 4);
    const size_t stage_need = off_cand + (size_t)n * sizeof(DevCand);
    if (e->sr_stage_bytes < stage_need) {
        if (e->sr_stage) {
            ENG_HIP(e, hipStreamSynchronize(s));
            eng_free(e, e->sr_stage);
            e->sr_stage = nullptr;
            e->sr_stage_bytes = 0;
        }
        const int st = eng_alloc_bytes(e, &e->sr_stage, stage_need);
        if (st != SABER_OK) return st;
        e->sr_stage_bytes = stage_need;
    }
    uint32_t* clean = (uint32_t*)e->sr_stage;
    int32_t* res = (int32_t*)((char*)e->sr_stage + off_res);   // count, keep[n], changed[n], area[n], box[4 n]
    int32_t *keep = res + 1, *changed = keep + n, *area = changed + n, *box = area + n;
    DevCand* cand = (DevCand*)((char*)e->sr_stage + off_cand);
    ENG_K(e, launch_small_regions(bits_in_dev, n, H, W, min_area, clean, changed, area, box, e->sr_ws, e->sr_ws_bytes, s));
    ENG_K(e, launch_small_regions_nms(changed, box, n, nms_thresh, cand, keep, res, clean, bits_out_dev, (int64_t)words, s));
    ENG_HIP(e, hipGetLastError());
    std::vector<int32_t> h((size_t)7 * n + 1);
    ENG_HIP(e, hipMemcpyAsync(h.data(), res, h.size() * 4, hipMemcpyDeviceToHost, s));
    ENG_HIP(e, hipStreamSynchronize(s));                        // the call's one synchronisation
    const int cnt = h[0];
    const int32_t *hk = h.data() + 1, *hc = hk + n, *ha = hc + n, *hb = ha + n;
    std::vector<saber_mask_meta> old(meta_host, meta_host + n);
    for (int i = 0; i < cnt; ++i) {
        const int k = hk[i];
        saber_mask_meta m = old[k];
        if (hc[k]) {
            m.area = ha[k];
            m.bbox_xywh[0] = (float)hb[4 * k]; m.bbox_xywh[1] = (float)hb[4 * k + 1];
            m.bbox_xywh[2] = (float)(hb[4 * k + 2] - hb[4 * k]); m.bbox_xywh[3] = (float)(hb[4 * k + 3] - hb[4 * k + 1]);
        }
        meta_host[i] = m;
    }
    *out_count = cnt;
    return SABER_OK;
}
