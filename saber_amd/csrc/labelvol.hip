// Propagated label volumes on the device: the stages between the video tracking loop and the 3-D stitch.
// SAM2Adapter.segment_volume (saber/adapters/sam2/predictor.py:232-348) paints every tracked object into a (Z,H,W) uint16 volume, drops
// (frame, object) pairs below the presence threshold, and the segmenters (saber/segmenters/propagation.py:87-160, tomo.py:205-258) merge
// the volumes of several seed slices.  All of it is label-indexed, one pass over the volume and bound by memory bandwidth:
//   lv_paint_stack_kernel   all n objects of a frame in one launch.  An output pixel computes its nearest source pixel once and scans the
//                           objects from the last to the first: the first logit above the threshold it meets is the one n successive
//                           paint_nearest launches would have left there, so a pixel reads only as many logits as it needs and is
//                           written at most once.  Labels travel by value (LV_PAINT_CHUNK per launch); a longer list goes in
//                           successive chunks in ascending order, which keeps the overwrite order.
//   lv_relabel_kernel       vol[z][i] = lut[z][vol[z][i]] in place.  A block stays within one frame, so its table row is uniform and is
//                           staged in LDS when it has at most LV_LUT_LDS entries (else it is read from global memory).  The body of a
//                           frame moves as 16-byte vectors; the elements in front of the first 16-byte boundary of the frame and behind
//                           its last one are handled one by one (a frame of an odd number of voxels starts off the boundary).  A vector
//                           that the table leaves unchanged is not written back.  The presence filter is this call with an
//                           identity-or-zero table.
//   lv_merge_max_kernel     acc = max(acc, binarize ? src > 0 : src), 16-byte vectors, unchanged vectors are not written back.
//   lv_merge_class_kernel   v = src[i]; 0 < v < L and conf[v] > best[i] (strictly): final[i] = cls[v], best[i] = conf[v].  A vector of eight
//                           background voxels costs its 16 bytes of src and nothing else.
// No atomics except the OR on paint's flag (as in paint_nearest_kernel): every output is exact and repeatable.  All offsets are 64-bit.
#include <algorithm>

#include "common.h"
#include "kernels.h"

#define LV_PAINT_CHUNK 64            // labels per launch of the stacked paint (128 bytes of kernel arguments)
#define LV_LUT_LDS 8192              // table entries a block of the relabel kernel stages in LDS (16 KB)

typedef uint16_t lv_u16x8 __attribute__((ext_vector_type(8)));
typedef float lv_f32x4 __attribute__((ext_vector_type(4)));

struct LvLabels { uint16_t v[LV_PAINT_CHUNK]; };

// (ys, xs) as in paint_nearest_kernel (video_ops.hip): floor((i + 0.5) * in / out) in double, clamped
__global__ __launch_bounds__(256) void lv_paint_stack_kernel(const float* __restrict__ logits, int n, int Hv, int Wv, float thr, LvLabels labels,
                                                             uint16_t* __restrict__ plane, int H, int W, int* __restrict__ any_flag) {
    const int64_t total = (int64_t)H * W, src_plane = (int64_t)Hv * Wv;
    bool hit = false;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int y = (int)(idx / W), x = (int)(idx - (int64_t)y * W);
        const int ys = min(max((int)floor(((double)y + 0.5) * Hv / H), 0), Hv - 1);
        const int xs = min(max((int)floor(((double)x + 0.5) * Wv / W), 0), Wv - 1);
        const float* p = logits + (int64_t)ys * Wv + xs;
        for (int i = n - 1; i >= 0; --i) {
            if (p[i * src_plane] > thr) {
                plane[idx] = labels.v[i];
                hit = true;
                break;
            }
        }
    }
    if (any_flag && __any(hit) && (threadIdx.x & 63) == 0) atomicOr(any_flag, 1);
}

const char* launch_paint_nearest_stack(const float* logits, int n, int Hv, int Wv, const int* labels_host, float thr, uint16_t* plane, int H, int W,
                                       int* any_flag, hipStream_t s) {
    if (n < 0 || Hv <= 0 || Wv <= 0 || H <= 0 || W <= 0) return "paint_nearest_stack: bad shape";
    if (n == 0) return nullptr;
    if (!logits || !labels_host || !plane) return "paint_nearest_stack: null pointer";
    for (int i = 0; i < n; ++i)
        if (labels_host[i] < 0 || labels_host[i] > 65535) return "paint_nearest_stack: label does not fit uint16";
    const int64_t total = (int64_t)H * W, src_plane = (int64_t)Hv * Wv;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
    for (int i0 = 0; i0 < n; i0 += LV_PAINT_CHUNK) {          // ascending chunks: a later chunk overwrites an earlier one, as later objects do
        const int m = std::min(LV_PAINT_CHUNK, n - i0);
        LvLabels lab;
        for (int i = 0; i < LV_PAINT_CHUNK; ++i) lab.v[i] = i < m ? (uint16_t)labels_host[i0 + i] : (uint16_t)0;
        hipLaunchKernelGGL(lv_paint_stack_kernel, dim3(blocks), dim3(256), 0, s, logits + (int64_t)i0 * src_plane, m, Hv, Wv, thr, lab, plane, H, W, any_flag);
    }
    return nullptr;
}

// ------------------------------------------------------------------------------------------------ per-frame table look-up
// One frame = blockIdx.x / bpf; the frame's blocks share its vectors, the frame's first block also takes the unaligned head and tail.
template <bool LDS>
__global__ __launch_bounds__(256) void lv_relabel_kernel(uint16_t* __restrict__ vol, int64_t HW, const uint16_t* __restrict__ lut, int L, int bpf) {
    __shared__ uint16_t tab[LDS ? LV_LUT_LDS : 1];
    const int64_t z = blockIdx.x / bpf;
    const int b = (int)(blockIdx.x - z * bpf);
    const uint16_t* row = lut + z * (int64_t)L;
    if (LDS) {
        for (int i = threadIdx.x; i < L; i += 256) tab[i] = row[i];
        __syncthreads();
    }
    auto map = [&](uint16_t v) -> uint16_t { return (int)v < L ? (LDS ? tab[v] : row[v]) : v; };
    uint16_t* f = vol + z * HW;
    // elements in front of the frame's first 16-byte boundary (addresses are 2-byte aligned: at most 7), then whole vectors, then the rest
    const int64_t head = min((int64_t)(((16u - (unsigned)((uintptr_t)f & 15u)) & 15u) >> 1), HW);
    const int64_t nvec = (HW - head) >> 3;
    const int64_t tail0 = head + (nvec << 3);
    lv_u16x8* body = reinterpret_cast<lv_u16x8*>(f + head);
    for (int64_t i = (int64_t)b * 256 + threadIdx.x; i < nvec; i += (int64_t)bpf * 256) {
        const lv_u16x8 v = body[i];
        lv_u16x8 r;
        bool changed = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) { r[j] = map(v[j]); changed |= r[j] != v[j]; }
        if (changed) body[i] = r;
    }
    if (b == 0) {
        const int64_t t = threadIdx.x;
        if (t < head) f[t] = map(f[t]);
        if (t < HW - tail0) f[tail0 + t] = map(f[tail0 + t]);       // fewer than 8 elements
    }
}

const char* launch_relabel_frames(uint16_t* vol, int Z, int64_t HW, const uint16_t* lut, int L, hipStream_t s) {
    if (Z <= 0 || HW <= 0) return "relabel_frames: bad shape";
    if (L <= 0) return "relabel_frames: the table must have at least one entry";
    if (!vol || !lut) return "relabel_frames: null pointer";
    if ((uintptr_t)vol & 1u) return "relabel_frames: the volume is not 2-byte aligned";
    // four vectors or more per thread, at most 128 blocks per frame
    const int bpf = (int)std::max<int64_t>(1, std::min<int64_t>(((HW >> 3) + 1023) / 1024, 128));
    if ((int64_t)Z * bpf > 0x7fffffff) return "relabel_frames: too many frames";
    const dim3 grid((unsigned)((int64_t)Z * bpf));
    if (L <= LV_LUT_LDS) hipLaunchKernelGGL(lv_relabel_kernel<true>, grid, dim3(256), 0, s, vol, HW, lut, L, bpf);
    else hipLaunchKernelGGL(lv_relabel_kernel<false>, grid, dim3(256), 0, s, vol, HW, lut, L, bpf);
    return nullptr;
}

// ------------------------------------------------------------------------------------------------ merging the volumes of several seed slices
namespace {
inline unsigned lv_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 8192)); }
inline bool lv_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
}  // namespace

// nvec vectors of 8 from element 0 (vec: both pointers are 16-byte aligned), the elements from 8 * nvec on one by one
__global__ __launch_bounds__(256) void lv_merge_max_kernel(uint16_t* __restrict__ acc, const uint16_t* __restrict__ src, int64_t n, int64_t nvec, int binarize) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    lv_u16x8* a8 = reinterpret_cast<lv_u16x8*>(acc);
    const lv_u16x8* s8 = reinterpret_cast<const lv_u16x8*>(src);
    for (int64_t i = t0; i < nvec; i += stride) {
        const lv_u16x8 a = a8[i], v = s8[i];
        lv_u16x8 r;
        bool changed = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint16_t w = binarize ? (uint16_t)(v[j] != 0) : v[j];
            r[j] = a[j] > w ? a[j] : w;
            changed |= r[j] != a[j];
        }
        if (changed) a8[i] = r;
    }
    for (int64_t i = (nvec << 3) + t0; i < n; i += stride) {
        const uint16_t v = src[i], w = binarize ? (uint16_t)(v != 0) : v;
        if (w > acc[i]) acc[i] = w;
    }
}

const char* launch_merge_max_u16(uint16_t* acc, const uint16_t* src, int64_t n, int binarize, hipStream_t s) {
    if (n < 0) return "merge_max_u16: bad element count";
    if (n == 0) return nullptr;
    if (!acc || !src) return "merge_max_u16: null pointer";
    const int64_t nvec = lv_aligned16(acc) && lv_aligned16(src) ? n >> 3 : 0;
    hipLaunchKernelGGL(lv_merge_max_kernel, dim3(lv_grid(nvec ? nvec : n)), dim3(256), 0, s, acc, src, n, nvec, binarize ? 1 : 0);
    return nullptr;
}

__device__ __forceinline__ void lv_class_one(uint16_t v, int L, const uint16_t* __restrict__ cls, const float* __restrict__ conf, uint16_t& fin, float& best) {
    if (v == 0 || (int)v >= L) return;
    const float c = conf[v];
    if (c > best) { fin = cls[v]; best = c; }
}

__global__ __launch_bounds__(256) void lv_merge_class_kernel(uint16_t* __restrict__ fin, float* __restrict__ best, const uint16_t* __restrict__ src,
                                                             const uint16_t* __restrict__ cls, const float* __restrict__ conf, int L, int64_t n, int64_t nvec) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const lv_u16x8* s8 = reinterpret_cast<const lv_u16x8*>(src);
    lv_u16x8* f8 = reinterpret_cast<lv_u16x8*>(fin);
    lv_f32x4* b4 = reinterpret_cast<lv_f32x4*>(best);
    for (int64_t i = t0; i < nvec; i += stride) {
        const lv_u16x8 v = s8[i];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) any |= v[j] != 0 && (int)v[j] < L;
        if (!any) continue;                                    // nothing to apply: final and best are not even read
        lv_u16x8 f = f8[i];
        lv_f32x4 b0 = b4[2 * i], b1 = b4[2 * i + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint16_t fa = f[j], fb = f[4 + j];
            float ba = b0[j], bb = b1[j];
            lv_class_one(v[j], L, cls, conf, fa, ba);
            lv_class_one(v[4 + j], L, cls, conf, fb, bb);
            f[j] = fa; f[4 + j] = fb; b0[j] = ba; b1[j] = bb;
        }
        f8[i] = f;
        b4[2 * i] = b0;
        b4[2 * i + 1] = b1;
    }
    for (int64_t i = (nvec << 3) + t0; i < n; i += stride) {
        uint16_t f = fin[i];
        float b = best[i];
        const uint16_t f_old = f;
        const float b_old = b;
        lv_class_one(src[i], L, cls, conf, f, b);
        if (f != f_old) fin[i] = f;
        if (b != b_old) best[i] = b;
    }
}

const char* launch_merge_class_conf(uint16_t* fin, float* best, const uint16_t* src, const uint16_t* cls, const float* conf, int L, int64_t n, hipStream_t s) {
    if (n < 0) return "merge_class_conf: bad element count";
    if (L <= 0) return "merge_class_conf: the tables must have at least one entry";
    if (n == 0) return nullptr;
    if (!fin || !best || !src || !cls || !conf) return "merge_class_conf: null pointer";
    const int64_t nvec = lv_aligned16(fin) && lv_aligned16(best) && lv_aligned16(src) ? n >> 3 : 0;
    hipLaunchKernelGGL(lv_merge_class_kernel, dim3(lv_grid(nvec ? nvec : n)), dim3(256), 0, s, fin, best, src, cls, conf, L, n, nvec);
    return nullptr;
}
