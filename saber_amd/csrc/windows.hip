// Sliding-window micrographs: the masks of saber2D.segment_image(use_sliding_window=True) (reference saber/segmenters/base.py:103-150) are
// window-sized.  rasterize_masks (:214-232) pastes each into a full-frame bool array and masks_to_array (saber/filters/masks.py:157-182)
// multiplies every one by its position + 1; here both run on the generator's bit-packed rows without leaving the device.
//
// A mask is a saber_window_mask record (include/saber_amd_kernels.h): h rows of w32 = ceil(w / 32) words at src + src_word, bit b of word k =
// window pixel 32k + b, pixel (0, 0) at frame pixel (y0, x0).  Bits at x >= w of a row's last word are not pixels and may hold anything.
//
// Frame word k of frame row y of a mask (window_word): with sx = 32k - x0 the source pixel of its bit 0 (negative left of the window),
// q = floor(sx / 32) and sh = sx - 32q in 0..31, the word is the 64-bit value (word q+1 : word q) of source row y - y0 shifted right by sh,
// where a word outside 0..w32-1 is zero and the row's last word is cut to its w - 32(w32 - 1) pixels.  So everything outside the window is
// zero by construction - also the bits at x >= W, which lie right of every window - sh = 0 (x0 a multiple of 32) reads one word and shifts
// nothing, and a window narrower than a word never reads the row below.
//   window_place_kernel  out[n][H][W32]: a lane per output word, consecutive lanes consecutive words; every word stored once (plain stores: no
//                        memset, no read-modify-write, no atomics).  Traffic floor: n H W32 4 B written + the window words read.
//   window_stack_kernel  out[count][H][W] of 1-, 2- or 4-byte elements, plane i = (label0 + i) where mask i covers the pixel: a lane per 16-byte
//                        piece (16 / 8 / 4 pixels, never across a frame word), stored as one uint4 when rows are 16-byte multiples on a
//                        16-byte aligned base, element by element otherwise.  Traffic floor: count H W elem B written.
// Both are grid-stride loops over 64-bit piece indices whose decomposition into (mask, row, piece) divides once per wave in 64 bits on
// the scalar side and twice per lane in 32 bits (a plane has fewer than 2^31 pieces); n never enters the grid's shape.
#include <algorithm>
#include <cstdio>
#include <string>

#include "../../include/saber_amd_kernels.h"
#include "engine.h"
#include "kernels.h"

namespace {

constexpr int WIN_BLOCK = 256;
constexpr int64_t WIN_MAX_BLOCKS = 2048;           // 256 CUs x 8 blocks; the rest of the work is walked by the grid-stride loop

// frame word k of frame row y of the mask of `rec` (see the head of the file)
__device__ __forceinline__ uint32_t window_word(const uint32_t* __restrict__ src, const saber_window_mask& rec, int y, int k) {
    const int ys = y - rec.y0;
    if (ys < 0 || ys >= rec.h) return 0u;
    const int w32 = (rec.w + 31) >> 5;
    const int sx = 32 * k - rec.x0;                // source pixel of bit 0
    const int q = sx >> 5;                         // arithmetic shift: floor
    const int sh = sx & 31;
    if (q >= w32 || q + 1 < 0) return 0u;
    const uint32_t* row = src + rec.src_word + (int64_t)ys * w32;
    const int tail = rec.w & 31;
    const uint32_t last_mask = tail ? (1u << tail) - 1u : 0xffffffffu;
    uint32_t lo = 0u, hi = 0u;
    if (q >= 0) lo = row[q] & (q == w32 - 1 ? last_mask : 0xffffffffu);
    if (sh != 0 && q + 1 < w32) hi = row[q + 1] & (q + 1 == w32 - 1 ? last_mask : 0xffffffffu);
    return (uint32_t)((((uint64_t)hi << 32) | (uint64_t)lo) >> sh);        // sh = 0: lo itself, never a shift by 32
}

// piece `idx` of planes of `per_plane` pieces in rows of `per_row`: the wave's first piece is divided in 64 bits once (wave-uniform),
// the lane's offset from it in 32 bits
struct WinPos { int64_t i; int y, p; };
__device__ __forceinline__ WinPos window_pos(int64_t wave_base, int lane, uint32_t per_plane, uint32_t per_row) {
    const int64_t i0 = wave_base / (int64_t)per_plane;
    const uint32_t r0 = (uint32_t)(wave_base - i0 * (int64_t)per_plane);
    const uint32_t r = r0 + (uint32_t)lane;        // < 2^31 + 64
    const uint32_t di = r / per_plane;
    const uint32_t rr = r - di * per_plane;
    WinPos o;
    o.i = i0 + di;
    o.y = (int)(rr / per_row);
    o.p = (int)(rr - (uint32_t)o.y * per_row);
    return o;
}

__device__ __forceinline__ int64_t window_wave_base(int64_t step) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    return ((int64_t)blockIdx.x + step * (int64_t)gridDim.x) * WIN_BLOCK + (int64_t)wave * 64;
}

__global__ __launch_bounds__(WIN_BLOCK) void window_place_kernel(const uint32_t* __restrict__ src, const saber_window_mask* __restrict__ table, int64_t total,
                                                                 int H, int W32, uint32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t per_plane = (uint32_t)H * (uint32_t)W32;
    for (int64_t step = 0;; ++step) {                              // wave-uniform
        const int64_t base = window_wave_base(step);
        if (base >= total) break;
        const int64_t idx = base + lane;
        if (idx < total) {
            const WinPos at = window_pos(base, lane, per_plane, (uint32_t)W32);
            const saber_window_mask rec = table[at.i];
            out[idx] = window_word(src, rec, at.y, at.p);
        }
    }
}

// the 16 bytes of P = 16 / ELEM pixels (the low P bits of `bits`) with value `label`
template <int ELEM> __device__ __forceinline__ uint4 window_expand(uint32_t bits, uint32_t label) {
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (ELEM == 1) {
            const uint32_t b = bits >> (4 * k);
            v[k] = ((b & 1u) | (((b >> 1) & 1u) << 8) | (((b >> 2) & 1u) << 16) | (((b >> 3) & 1u) << 24)) * label;     // label <= 255: no carry between bytes
        } else if (ELEM == 2) {
            const uint32_t b = bits >> (2 * k);
            v[k] = ((b & 1u) | (((b >> 1) & 1u) << 16)) * label;                                                       // label <= 65535
        } else {
            v[k] = ((bits >> k) & 1u) * label;
        }
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}

template <int ELEM, typename T>
__global__ __launch_bounds__(WIN_BLOCK) void window_stack_kernel(const uint32_t* __restrict__ src, const saber_window_mask* __restrict__ table, int64_t total,
                                                                 uint32_t label0, int H, int W, int per_row, bool vec, T* __restrict__ out) {
    constexpr int P = 16 / ELEM;                                   // pixels of a piece; P divides 32: a piece lies inside one frame word
    const int lane = threadIdx.x & 63;
    const uint32_t per_plane = (uint32_t)H * (uint32_t)per_row;
    for (int64_t step = 0;; ++step) {                              // wave-uniform
        const int64_t base = window_wave_base(step);
        if (base >= total) break;
        if (base + lane < total) {
            const WinPos at = window_pos(base, lane, per_plane, (uint32_t)per_row);
            const saber_window_mask rec = table[at.i];
            const int x = at.p * P;
            const uint32_t bits = window_word(src, rec, at.y, x >> 5) >> (x & 31);
            const uint32_t label = label0 + (uint32_t)at.i;
            T* o = out + (at.i * H + at.y) * (int64_t)W + x;
            if (vec) {
                *reinterpret_cast<uint4*>(o) = window_expand<ELEM>(bits, label);
            } else {
                const int lim = min(P, W - x);
                for (int k = 0; k < lim; ++k) o[k] = (T)(((bits >> k) & 1u) * label);
            }
        }
    }
}

unsigned window_blocks(int64_t total) { return (unsigned)std::min<int64_t>((total + WIN_BLOCK - 1) / WIN_BLOCK, WIN_MAX_BLOCKS); }

const char* window_shape_error(const char* who, int H, int W, char* msg, size_t msg_len) {
    if (H < 1 || W < 1) {
        snprintf(msg, msg_len, "%s: H and W must be at least 1", who);
        return msg;
    }
    if ((int64_t)H * W >= ((int64_t)1 << 31)) {
        snprintf(msg, msg_len, "%s: frames of 2^31 pixels or more are not supported", who);
        return msg;
    }
    return nullptr;
}

const char* window_stack_error(int first, int count, int elem_bytes, char* msg, size_t msg_len) {
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) {
        snprintf(msg, msg_len, "window_label_stack: elem_bytes must be 1, 2 or 4, got %d", elem_bytes);
        return msg;
    }
    if (first < 0 || count < 0) {
        snprintf(msg, msg_len, "window_label_stack: first and count must not be negative");
        return msg;
    }
    const int64_t top = (int64_t)first + count;                    // the largest value written
    if (top > 0x7fffffff || (elem_bytes == 1 && top > 255) || (elem_bytes == 2 && top > 65535)) {
        snprintf(msg, msg_len, "window_label_stack: label %lld (first + count) does not fit an element of %d byte%s", (long long)top, elem_bytes,
                 elem_bytes == 1 ? "" : "s");
        return msg;
    }
    return nullptr;
}

}  // namespace

const char* launch_window_place(const uint32_t* src, const saber_window_mask* table, int n, int H, int W, uint32_t* out, hipStream_t s) {
    static thread_local char msg[160];
    if (n < 0) return "place_window_masks: n must not be negative";
    if (const char* e = window_shape_error("place_window_masks", H, W, msg, sizeof msg)) return e;
    if (n == 0) return nullptr;
    if (!src || !table || !out) return "place_window_masks: null pointer";
    if (((uintptr_t)src & 3u) || ((uintptr_t)out & 3u) || ((uintptr_t)table & 7u)) return "place_window_masks: src and out must be 4-byte, the table 8-byte aligned";
    const int W32 = (W + 31) / 32;
    const int64_t total = (int64_t)n * H * W32;
    hipLaunchKernelGGL(window_place_kernel, dim3(window_blocks(total)), dim3(WIN_BLOCK), 0, s, src, table, total, H, W32, out);
    return nullptr;
}

// `t`: the record of the first plane, which is painted label0
static const char* window_stack_go(const uint32_t* src, const saber_window_mask* t, uint32_t label0, int count, int H, int W, int elem_bytes, void* out,
                                   hipStream_t s) {
    if (!src || !t || !out) return "window_label_stack: null pointer";
    if (((uintptr_t)src & 3u) || ((uintptr_t)out & (uintptr_t)(elem_bytes - 1)) || ((uintptr_t)t & 7u))
        return "window_label_stack: src must be 4-byte, out element and the table 8-byte aligned";
    const int P = 16 / elem_bytes;
    const int per_row = (W + P - 1) / P;
    const int64_t total = (int64_t)count * H * per_row;
    const bool vec = ((int64_t)W * elem_bytes) % 16 == 0 && ((uintptr_t)out & 15u) == 0;
    const dim3 grid(window_blocks(total)), block(WIN_BLOCK);
    if (elem_bytes == 1) hipLaunchKernelGGL((window_stack_kernel<1, uint8_t>), grid, block, 0, s, src, t, total, label0, H, W, per_row, vec, (uint8_t*)out);
    else if (elem_bytes == 2) hipLaunchKernelGGL((window_stack_kernel<2, uint16_t>), grid, block, 0, s, src, t, total, label0, H, W, per_row, vec, (uint16_t*)out);
    else hipLaunchKernelGGL((window_stack_kernel<4, uint32_t>), grid, block, 0, s, src, t, total, label0, H, W, per_row, vec, (uint32_t*)out);
    return nullptr;
}

const char* launch_window_stack(const uint32_t* src, const saber_window_mask* table, int first, int count, int H, int W, int elem_bytes, void* out,
                                hipStream_t s) {
    static thread_local char msg[160];
    if (const char* e = window_stack_error(first, count, elem_bytes, msg, sizeof msg)) return e;
    if (const char* e = window_shape_error("window_label_stack", H, W, msg, sizeof msg)) return e;
    if (count == 0) return nullptr;
    if (!table) return "window_label_stack: null pointer";
    return window_stack_go(src, table + first, (uint32_t)first + 1u, count, H, W, elem_bytes, out, s);
}

// ------------------------------------------------------------------------------------------------ engine entries (include/saber_amd.h)
// every record inside the frame and inside src; the message names the first one that is not
static int window_check_table(saber_engine* e, const char* who, const saber_window_mask* t, int n, int H, int W, int64_t src_words) {
    for (int i = 0; i < n; ++i) {
        const saber_window_mask& r = t[i];
        const char* what = nullptr;
        if (r.h < 1 || r.w < 1) what = "h and w must be at least 1";
        else if (r.y0 < 0 || (int64_t)r.y0 + r.h > H) what = "rows y0 .. y0 + h leave the frame";
        else if (r.x0 < 0 || (int64_t)r.x0 + r.w > W) what = "columns x0 .. x0 + w leave the frame";
        else if (r.src_word < 0 || r.src_word > src_words || (int64_t)r.h * ((r.w + 31) / 32) > src_words - r.src_word) what = "its words leave src";
        if (what) {
            char msg[256];
            snprintf(msg, sizeof msg, "%s: record %d (src_word %lld, y0 %d, x0 %d, h %d, w %d; frame %d x %d, src of %lld words): %s", who, i,
                     (long long)r.src_word, r.y0, r.x0, r.h, r.w, H, W, (long long)src_words, what);
            return eng_fail(e, SABER_ERR_INVALID, msg);
        }
    }
    return SABER_OK;
}

// records [first, first + count) of the host table on the device, behind whatever `s` holds.  A table that outgrows the buffer gets a new
// one of twice the size; the old one stays with the handle until it is destroyed (a launch in flight may still read it, and releasing it
// would wait for the device).
static int window_upload(saber_engine* e, const saber_window_mask* t, int first, int count, hipStream_t s, const saber_window_mask** out) {
    if (e->win_table_cap < (size_t)count) {
        const size_t cap = std::max<size_t>((size_t)count, 2 * e->win_table_cap);
        void* p = nullptr;
        const int st = eng_alloc_bytes(e, &p, cap * sizeof(saber_window_mask));
        if (st != SABER_OK) return st;
        e->win_table_dev = p;
        e->win_table_cap = cap;
    }
    ENG_HIP(e, hipMemcpyAsync(e->win_table_dev, t + first, sizeof(saber_window_mask) * (size_t)count, hipMemcpyHostToDevice, s));
    *out = (const saber_window_mask*)e->win_table_dev;
    return SABER_OK;
}

extern "C" int saber_place_window_masks(saber_engine* e, const uint32_t* src_dev, int64_t src_words, const saber_window_mask* table_host, int n, int H, int W,
                                        uint32_t* out_dev, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    char msg[160];
    if (n < 0 || src_words < 0) return eng_fail(e, SABER_ERR_INVALID, "place_window_masks: n and src_words must not be negative");
    if (const char* m = window_shape_error("place_window_masks", H, W, msg, sizeof msg)) return eng_fail(e, SABER_ERR_INVALID, m);
    if (n == 0) return SABER_OK;
    if (!src_dev || !table_host || !out_dev) return eng_fail(e, SABER_ERR_INVALID, "place_window_masks: null pointer");
    const int st = window_check_table(e, "place_window_masks", table_host, n, H, W, src_words);
    if (st != SABER_OK) return st;
    ENG_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const saber_window_mask* td = nullptr;
    const int up = window_upload(e, table_host, 0, n, s, &td);
    if (up != SABER_OK) return up;
    ENG_KP(e, PC_ELEMENTWISE, 0.0, (double)n * H * ((W + 31) / 32) * 4.0, launch_window_place(src_dev, td, n, H, W, out_dev, s));
    ENG_HIP(e, hipGetLastError());
    return SABER_OK;
}

extern "C" int saber_window_label_stack(saber_engine* e, const uint32_t* src_dev, int64_t src_words, const saber_window_mask* table_host, int n, int first,
                                        int count, int H, int W, int elem_bytes, void* out_dev, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    char msg[160];
    if (n < 0 || src_words < 0) return eng_fail(e, SABER_ERR_INVALID, "window_label_stack: n and src_words must not be negative");
    if (const char* m = window_stack_error(first, count, elem_bytes, msg, sizeof msg)) return eng_fail(e, SABER_ERR_INVALID, m);
    if ((int64_t)first + count > n) return eng_fail(e, SABER_ERR_INVALID, "window_label_stack: first + count exceeds the " + std::to_string(n) + " records of the table");
    if (const char* m = window_shape_error("window_label_stack", H, W, msg, sizeof msg)) return eng_fail(e, SABER_ERR_INVALID, m);
    if (n > 0 && !table_host) return eng_fail(e, SABER_ERR_INVALID, "window_label_stack: null pointer");
    const int st = window_check_table(e, "window_label_stack", table_host, n, H, W, src_words);
    if (st != SABER_OK) return st;
    if (count == 0) return SABER_OK;
    if (!src_dev || !out_dev) return eng_fail(e, SABER_ERR_INVALID, "window_label_stack: null pointer");
    ENG_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const saber_window_mask* td = nullptr;
    const int up = window_upload(e, table_host, first, count, s, &td);
    if (up != SABER_OK) return up;
    ENG_KP(e, PC_ELEMENTWISE, 0.0, (double)count * H * W * elem_bytes, window_stack_go(src_dev, td, (uint32_t)first + 1u, count, H, W, elem_bytes, out_dev, s));
    ENG_HIP(e, hipGetLastError());
    return SABER_OK;
}
