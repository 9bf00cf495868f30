// Slab preparation of tomoSegmenter.segment_vol on the device (reference: saber/segmenters/tomo.py:98-101): the z Gaussian of
// saber.filters.gaussian.gaussian_smoothing (filters/gaussian.py:17-74, conv1d with zero 'same' padding), preprocess.normalize
// (utils/preprocessing.py:20-37, rgb=False) and preprocess.project_tomogram (:39-65).  Two streaming passes over the volume and one over a slab:
//   vp_corr_window_kernel   correlation along one axis of a (outer, len, inner) view, inner > 1 (dims 0 and 1 of a volume).  Lanes run along
//                           `inner` (V = VP_V = 4 elements per lane: 16-byte stores, and 16 / 8 / 4-byte loads for fp32 / 16-bit / 8-bit input, when
//                           inner is a multiple of 4 and the pointers are aligned; else V = 1), a thread walks `len` in blocks of VP_B outputs
//                           and keeps the last KS - 1 inputs in registers, so an input element is read once per chunk.  `len` is cut into
//                           chunks (grid.y) with a KS - 1 halo, so that a small `inner` still gives the device enough threads.  Every load is
//                           unconditional on a clamped row and the padding is a select afterwards: no branch around a load.
//   vp_corr_direct_kernel   one output per thread, KS taps read straight from memory: inner = 1 (dim 2, where the taps of neighbouring
//                           lanes share cache lines) and every tap count the window kernel is not instantiated for.
// Both evaluate acc = 0; acc = fmaf(w[k], x[l + k - KS/2], acc) for k = 0 .. KS-1 in that order, padding as x = 0, so they agree bit
// for bit, with each other and across input types (the widening to fp32 is exact for all four).  A window of zeros gives exactly 0.
// Optionally both leave min / max of what they wrote: per-thread fminf / fmaxf, a block reduction, then one pair of 32-bit atomic
// maxima per block on order-preserving keys (the minimum as the maximum of the complemented key, so that the two words start from one
// memset); vp_minmax_decode_kernel turns the keys into the two floats in place.
//   vp_normalize_kernel     v <- (v - lo) / ((hi - lo) + 1e-8f) in place, lo / hi read from device memory, IEEE division.
//   vp_project_kernel       out = (x[z0] + x[z0+1] + ... + x[z1-1]) / float(z1 - z0): sequential fp32 sum in ascending z, one IEEE division.
// All offsets are 64-bit.
#include <algorithm>

#include "common.h"
#include "kernels.h"

#ifndef VP_B
#define VP_B 8                        // outputs per register block of the window kernel; chunk lengths are multiples of it
#endif
#ifndef VP_V
#define VP_V 4                        // voxels per lane of the wide form (make EXTRA="-DVP_V=2 -DVP_B=16" builds another: measured, no gain)
#endif
#define VP_MIN_CHUNK 32               // shortest automatic chunk: the halo re-reads (KS - 1) / chunk of the input
#define VP_TARGET_THREADS (1 << 18)   // 256 CUs x 4 SIMDs x 4 waves x 64 lanes: `len` is only split while there are fewer threads

struct VpTaps { float w[VP_MAX_KS]; };

template <typename T, int V> struct VpVec { typedef T type __attribute__((ext_vector_type(V))); };

// V elements at p as fp32
template <typename T, int V>
__device__ __forceinline__ void vp_load(const T* __restrict__ p, float (&o)[V]) {
    if constexpr (V == 1) {
        o[0] = (float)p[0];
    } else {
        const typename VpVec<T, V>::type v = *reinterpret_cast<const typename VpVec<T, V>::type*>(p);
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (float)v[j];
    }
}

__device__ __forceinline__ uint32_t vp_key(float f) {       // ascending in f for every non-NaN f
    const uint32_t u = __float_as_uint(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float vp_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

// min / max over the block's threads, then one pair of atomics; keys[0] = max of ~key(min), keys[1] = max of key(max)
__device__ __forceinline__ void vp_block_minmax(float lo, float hi, uint32_t* keys) {
    __shared__ float part[2][4];
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = lo; part[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(part[0][0], part[0][1]), fminf(part[0][2], part[0][3]));
        hi = fmaxf(fmaxf(part[1][0], part[1][1]), fmaxf(part[1][2], part[1][3]));
        if (lo <= hi) {                                      // the block wrote at least one number
            atomicMax(&keys[0], ~vp_key(lo));
            atomicMax(&keys[1], vp_key(hi));
        }
    }
}

__global__ void vp_minmax_decode_kernel(uint32_t* keys) {
    const uint32_t a = keys[0], b = keys[1];
    reinterpret_cast<float*>(keys)[0] = vp_unkey(~a);
    reinterpret_cast<float*>(keys)[1] = vp_unkey(b);
}

// ------------------------------------------------------------------------------------------------ correlation, register window
// cols = outer * (inner / V) threads along grid.x, chunk blockIdx.y of `len`
template <typename T, int KS, int V>
__global__ __launch_bounds__(256) void vp_corr_window_kernel(const T* __restrict__ in, float* __restrict__ out, int64_t len, int64_t inner, int64_t cols,
                                                             int chunk, VpTaps taps, uint32_t* keys) {
    constexpr int R = KS / 2;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    if (col < cols) {
        const int64_t groups = inner / V;
        const int64_t base = (col / groups) * len * inner + (col % groups) * V;
        const T* __restrict__ src = in + base;
        float* __restrict__ dst = out + base;
        const int64_t l0 = (int64_t)blockIdx.y * chunk, l1 = min(l0 + chunk, len);
        float v[KS - 1 + VP_B][V];                           // v[m] = x[lb - R + m]
#pragma unroll
        for (int m = 0; m < KS - 1; ++m) {
            const int64_t p = l0 - R + m;
            vp_load<T, V>(src + min(max(p, (int64_t)0), len - 1) * inner, v[m]);
            const bool pad = p < 0 || p >= len;
#pragma unroll
            for (int j = 0; j < V; ++j) v[m][j] = pad ? 0.f : v[m][j];
        }
        for (int64_t lb = l0; lb < l1; lb += VP_B) {
#pragma unroll
            for (int b = 0; b < VP_B; ++b) {
                const int64_t p = lb + R + b;
                vp_load<T, V>(src + min(p, len - 1) * inner, v[KS - 1 + b]);
                const bool pad = p >= len;
#pragma unroll
                for (int j = 0; j < V; ++j) v[KS - 1 + b][j] = pad ? 0.f : v[KS - 1 + b][j];
            }
#pragma unroll
            for (int b = 0; b < VP_B; ++b) {
                if (lb + b < l1) {
                    float acc[V];
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
#pragma unroll
                        for (int j = 0; j < V; ++j) acc[j] = fmaf(taps.w[k], v[b + k][j], acc[j]);
                    }
                    float* q = dst + (lb + b) * inner;
                    if constexpr (V > 1) {
                        typename VpVec<float, V>::type r;
#pragma unroll
                        for (int j = 0; j < V; ++j) r[j] = acc[j];
                        *reinterpret_cast<typename VpVec<float, V>::type*>(q) = r;
                    } else {
#pragma unroll
                        for (int j = 0; j < V; ++j) q[j] = acc[j];
                    }
#pragma unroll
                    for (int j = 0; j < V; ++j) { lo = fminf(lo, acc[j]); hi = fmaxf(hi, acc[j]); }
                }
            }
#pragma unroll
            for (int m = 0; m < KS - 1; ++m) {
#pragma unroll
                for (int j = 0; j < V; ++j) v[m][j] = v[m + VP_B][j];
            }
        }
    }
    if (keys) vp_block_minmax(lo, hi, keys);
}

// ------------------------------------------------------------------------------------------------ correlation, one output per thread
template <typename T>
__global__ __launch_bounds__(256) void vp_corr_direct_kernel(const T* __restrict__ in, float* __restrict__ out, int64_t total, int64_t len, int64_t inner,
                                                             int ks, VpTaps taps, uint32_t* keys) {
    const int r = ks / 2;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t l = (idx / inner) % len;
        const T* __restrict__ src = in + (idx - l * inner);     // row 0 of this output's column
        float acc = 0.f;
        for (int k = 0; k < ks; ++k) {
            const int64_t p = l + k - r;
            const float x = (float)src[min(max(p, (int64_t)0), len - 1) * inner];
            acc = fmaf(taps.w[k], (p < 0 || p >= len) ? 0.f : x, acc);
        }
        out[idx] = acc;
        lo = fminf(lo, acc);
        hi = fmaxf(hi, acc);
    }
    if (keys) vp_block_minmax(lo, hi, keys);
}

// ------------------------------------------------------------------------------------------------ normalise, project
// n4 float4 groups (0 when v is not 16-byte aligned), then the scalars from 4 * n4 on
__global__ __launch_bounds__(256) void vp_normalize_kernel(float* __restrict__ v, int64_t n, int64_t n4, const float* __restrict__ minmax) {
    const float lo = minmax[0], hi = minmax[1];
    const float d = __fadd_rn(__fsub_rn(hi, lo), 1e-8f);
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    for (int64_t i = t; i < n4; i += stride) {
        f32x4 x = v4[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = __fdiv_rn(__fsub_rn(x[j], lo), d);
        v4[i] = x;
    }
    for (int64_t i = 4 * n4 + t; i < n; i += stride) v[i] = __fdiv_rn(__fsub_rn(v[i], lo), d);
}

template <int V>
__global__ __launch_bounds__(256) void vp_project_kernel(const float* __restrict__ vol, int64_t plane, int z0, int z1, float* __restrict__ out) {
    const float cnt = (float)(z1 - z0);
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < plane; i += (int64_t)gridDim.x * 256 * V) {
        const float* __restrict__ p = vol + (int64_t)z0 * plane + i;
        float acc[V];
        vp_load<float, V>(p, acc);
#pragma unroll 4
        for (int z = z0 + 1; z < z1; ++z) {
            p += plane;
            float x[V];
            vp_load<float, V>(p, x);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = __fadd_rn(acc[j], x[j]);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = __fdiv_rn(acc[j], cnt);
        if constexpr (V == 4) {
            const f32x4 r = {acc[0], acc[1], acc[2], acc[3]};
            *reinterpret_cast<f32x4*>(out + i) = r;
        } else {
            out[i] = acc[0];
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
namespace {
inline bool vp_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
inline unsigned vp_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1 << 20)); }

template <typename T>
const char* vp_correlate(const T* in, float* out, int64_t outer, int64_t len, int64_t inner, const VpTaps& taps, int ks, int chunk_len, uint32_t* keys,
                         hipStream_t s) {
    if (ks != 15 || inner == 1) {
        const int64_t total = outer * len * inner;
        hipLaunchKernelGGL(vp_corr_direct_kernel<T>, dim3(vp_grid(total)), dim3(256), 0, s, in, out, total, len, inner, ks, taps, keys);
        return nullptr;
    }
    const bool vec = (inner % VP_V) == 0 && vp_aligned(in, VP_V * sizeof(T)) && vp_aligned(out, VP_V * sizeof(float));
    const int64_t cols = outer * (vec ? inner / VP_V : inner);
    int64_t chunk = chunk_len;
    if (chunk <= 0) {          // split `len` only as far as the device needs more threads
        const int64_t want = std::max<int64_t>(1, VP_TARGET_THREADS / cols);
        const int64_t nch = std::max<int64_t>(1, std::min<int64_t>(want, (len + VP_MIN_CHUNK - 1) / VP_MIN_CHUNK));
        chunk = (len + nch - 1) / nch;
    }
    chunk = std::min<int64_t>((chunk + VP_B - 1) / VP_B * VP_B, (int64_t)1 << 30);
    const int64_t nch = (len + chunk - 1) / chunk, gx = (cols + 255) / 256;
    if (nch > 65535) return "correlate1d_zero: chunk_len gives more than 65535 chunks";
    if (gx > 0x7fffffff) return "correlate1d_zero: more than 2^39 columns";
    const dim3 grid((unsigned)gx, (unsigned)nch);
    if (vec) hipLaunchKernelGGL((vp_corr_window_kernel<T, 15, VP_V>), grid, dim3(256), 0, s, in, out, len, inner, cols, (int)chunk, taps, keys);
    else hipLaunchKernelGGL((vp_corr_window_kernel<T, 15, 1>), grid, dim3(256), 0, s, in, out, len, inner, cols, (int)chunk, taps, keys);
    return nullptr;
}
}  // namespace

const char* launch_correlate1d_zero(const void* in, int dtype, float* out, int64_t outer, int64_t len, int64_t inner, const float* taps, int ks,
                                    int chunk_len, float* minmax, hipStream_t s) {
    if (!in || !out || !taps || outer <= 0 || len <= 0 || inner <= 0 || chunk_len < 0) return "correlate1d_zero: bad argument";
    if (ks < 3 || ks > VP_MAX_KS || (ks & 1) == 0) return "correlate1d_zero: ks must be odd and in 3..63";
    if (dtype < 0 || dtype > 3) return "correlate1d_zero: dtype must be 0 (float32), 1 (int16), 2 (uint16) or 3 (uint8)";
    if ((const void*)out == in) return "correlate1d_zero: the output must be a separate buffer";
    if (outer > INT64_MAX / len || outer * len > INT64_MAX / inner / 4) return "correlate1d_zero: the array is too large";
    VpTaps t;
    for (int k = 0; k < VP_MAX_KS; ++k) t.w[k] = k < ks ? taps[k] : 0.f;
    uint32_t* keys = reinterpret_cast<uint32_t*>(minmax);
    if (keys && hipMemsetAsync(keys, 0, 8, s) != hipSuccess) return "correlate1d_zero: hipMemsetAsync failed";
    const char* m = dtype == 0 ? vp_correlate((const float*)in, out, outer, len, inner, t, ks, chunk_len, keys, s)
                  : dtype == 1 ? vp_correlate((const int16_t*)in, out, outer, len, inner, t, ks, chunk_len, keys, s)
                  : dtype == 2 ? vp_correlate((const uint16_t*)in, out, outer, len, inner, t, ks, chunk_len, keys, s)
                               : vp_correlate((const uint8_t*)in, out, outer, len, inner, t, ks, chunk_len, keys, s);
    if (m) return m;
    if (keys) hipLaunchKernelGGL(vp_minmax_decode_kernel, dim3(1), dim3(1), 0, s, keys);
    return nullptr;
}

const char* launch_normalize_minmax(float* v, int64_t n, const float* minmax, hipStream_t s) {
    if (!v || !minmax || n <= 0) return "normalize_minmax: bad argument";
    const int64_t n4 = vp_aligned(v, 16) ? n / 4 : 0;
    hipLaunchKernelGGL(vp_normalize_kernel, dim3(vp_grid(std::max<int64_t>(n4, n - 4 * n4))), dim3(256), 0, s, v, n, n4, minmax);
    return nullptr;
}

const char* launch_project_mean(const float* vol, int Z, int H, int W, int z0, int z1, float* out, hipStream_t s) {
    if (!vol || !out || Z <= 0 || H <= 0 || W <= 0) return "project_mean: bad argument";
    if (z0 < 0 || z1 > Z || z1 <= z0) return "project_mean: the range z0 .. z1-1 must be non-empty and inside the volume";
    const int64_t plane = (int64_t)H * W;
    if (plane % 4 == 0 && vp_aligned(vol, 16) && vp_aligned(out, 16))
        hipLaunchKernelGGL(vp_project_kernel<4>, dim3(vp_grid(plane / 4)), dim3(256), 0, s, vol, plane, z0, z1, out);
    else
        hipLaunchKernelGGL(vp_project_kernel<1>, dim3(vp_grid(plane)), dim3(256), 0, s, vol, plane, z0, z1, out);
    return nullptr;
}
