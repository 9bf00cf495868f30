// Per-label adaptive 3-D Gaussian smoothing of the stitched label volume on the device.
// Replaces saber.filters.masks.fast_3d_gaussian_smoothing (saber/filters/masks.py:230-287) and the separable filter under it,
// saber.filters.gaussian.gaussian_smoothing_3d (saber/filters/gaussian.py:76-138): the step segment_tomogram_core applies to the
// segmenter's output before it is written (saber/entry_points/inference_core.py:68-74, scale = 0.05).  For every label value v != 0,
// ascending: mask = (volume == v); sigma = scale * 2 * (3 |mask| / 4 pi)^(1/3) (masks.py:289-309); taps = normalised
// exp(-i^2 / 2 sigma^2), i in [-r, r], 2r+1 = int(6 sigma + 1) made odd (gaussian.py:97-104); zero-padded 1-D convolutions along
// x, then y, then z in fp32 (gaussian.py:110-131); result[field > 0.5] = (uint8) v, later labels overwriting earlier ones.
//
// The reference convolves the WHOLE volume three times per label.  Here a label only costs its bounding box: outside the box
// (say beyond its last x) at most the taps of one side of the kernel can meet the mask, and those sum to (1 - tap0) / 2 < 0.5, so the
// field cannot pass the threshold there; and along an axis that has been convolved the other two still see zeros outside the box.
//   1. sm_max / sm_stats   largest label value; voxel count + bounding box per label value (one atomic set per wave and label)
//   2. host                sigma, radius, taps per present label (double / float arithmetic as the reference's numpy / torch lines)
//   3. sm_conv_x           T1 = conv_x(volume == v) on the box, all labels of a group in one launch; rows come through a segment table
//   4. sm_conv_axis<0>     T2 = conv_y(T1)
//   5. sm_conv_axis<1>     field = conv_z(T2) on the box's own planes; field > 0.5 -> atomicMax(winner, v)   ("later label overwrites" =
//                          largest label)
//   6. sm_cast             out = (uint8) winner  (the reference's result array is uint8: label values wrap modulo 256)
// HBM-bound byte work: ~20 B per box voxel.  Each output sums its taps in ascending tap order with fma, as the CPU oracle does.
// Steps 3-6 are sm_convolve, the one pipeline behind every entry point.
//
// One z-chunk of a volume that is spread over several ranks (saber_smooth_labels_chunk, at the end of this file): steps 1-2 on (planes
// below, own planes, planes above) in three buffers, with the counts of the whole volume handed in, then the same sm_convolve: the
// segment table names the three buffers, a box's own planes are those of the chunk, and the winner covers the own planes only.  The
// whole volume (sm_run) is the chunk without halos: one segment, every box written on all its planes, output plane 0 = volume plane 0.
// So both routes sum every output with the same instructions.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "common.h"
#include "engine.h"

struct SmLabel {
    uint32_t label;
    int z0, y0, x0, dz, dy, dx;
    int r;              // kernel radius, taps = 2r+1
    int tap_off;        // first tap in the tap table (preceded and followed by SM_OPT-1 zeros)
    int64_t ws_off;     // T1 at ws + ws_off, T2 at ws + ws_off + dz*dy*dx (floats)
};

#define SM_OPT 8        // outputs per thread along the convolved axis (sm_conv_axis)
#define SM_TL 32        // outputs per block along the convolved axis
#define SM_TX 64        // x columns per block

// ZFLAG (both kernels): only the planes whose z flag is set count (morph3d.hip: organelles count where there is membrane)
template <typename T, bool ZFLAG>
__global__ __launch_bounds__(256) void sm_max_kernel(const T* __restrict__ lab, const uint8_t* __restrict__ zflag, int64_t plane, int64_t n,
                                                     uint32_t* __restrict__ out) {
    uint32_t m = 0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256)
        if (!ZFLAG || zflag[v / plane]) m = max(m, (uint32_t)lab[v]);
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// stats[v] = {count, zmin, ymin, xmin, zmax, ymax, xmax, -}; one wave per 512-voxel piece of a row, 8 voxels per lane.
template <typename T, bool ZFLAG>
__global__ __launch_bounds__(256) void sm_stats_kernel(const T* __restrict__ lab, const uint8_t* __restrict__ zflag, int W, int64_t rows, int H,
                                                       uint32_t* __restrict__ stats) {
    const int chunks = (W + 511) / 512;
    const int64_t piece = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (piece >= rows * chunks) return;
    const int64_t row = piece / chunks;
    const uint32_t z = (uint32_t)(row / H), y = (uint32_t)(row % H);
    if (ZFLAG && !zflag[z]) return;                             // wave-uniform
    const int lane = threadIdx.x & 63;
    const int xb = (int)(piece % chunks) * 512 + lane * 8;
    const T* p = lab + row * W;
    // runs inside this lane's 8 voxels; a run is flushed through the wave: lanes holding the same label combine first
    uint32_t cur = 0, cnt = 0, xlo = 0, xhi = 0;
    for (int i = 0; i <= 8; ++i) {
        const int x = xb + i;
        const uint32_t v = (i < 8 && x < W) ? (uint32_t)p[x] : 0u;
        const bool flush = (v != cur);
        uint32_t pend = (flush && cur) ? cur : 0u;              // label to flush now (0 = nothing)
        while (true) {
            const uint64_t any = __ballot(pend != 0);
            if (!any) break;
            const int leader = __ffsll((long long)any) - 1;
            const uint32_t lv = (uint32_t)__shfl((int)pend, leader, 64);
            const bool mine = (pend == lv);
            uint32_t c = mine ? cnt : 0u, lo = mine ? xlo : 0xffffffffu, hi = mine ? xhi : 0u;
            for (int o = 32; o > 0; o >>= 1) {                  // one ladder for the three: their shuffles of a step are in flight together
                c += (uint32_t)__shfl_xor((int)c, o, 64);
                lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
                hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
            }
            if (lane == leader) {
                uint32_t* s = stats + (size_t)lv * 8;
                atomicAdd(s + 0, c);
                atomicMin(s + 1, z); atomicMin(s + 2, y); atomicMin(s + 3, lo);
                atomicMax(s + 4, z); atomicMax(s + 5, y); atomicMax(s + 6, hi);
            }
            if (mine) pend = 0;
        }
        if (flush) { cur = v; cnt = 0; xlo = (uint32_t)x; }
        if (v) { ++cnt; xhi = (uint32_t)x; }
    }
}

// block -> (label of the group, tile): prefix[i] = tiles of labels < i (uniform binary search, scalar loads)
__device__ __forceinline__ int sm_find(const int* __restrict__ prefix, int n, int b) {
    int lo = 0, hi = n;                                         // prefix[lo] <= b < prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// The planes of a volume in up to three buffers (saber_smooth_labels_chunk: the planes below, the own planes, the planes above).  Planes
// are counted from the first plane of the first buffer; plane p lies in the last segment whose first[] <= p.  A whole volume is one
// segment: first = {0, INT_MAX, INT_MAX}.
struct SmSegs {
    const void* base[3];
    int first[3];
};

// T1[z][y][x] = sum_k taps[k] * (vol[z0+z][y0+y][x0+x+k-r] == label), x+k-r inside the box.  4 waves = 4 rows of the box, 64 x each.
// The row pointer comes from the segment table (two wave-uniform selects).
template <typename T>
__global__ __launch_bounds__(256) void sm_conv_x_kernel(SmSegs segs, int H, int W, const SmLabel* __restrict__ labels,
                                                        const int* __restrict__ prefix, int n_labels, const float* __restrict__ taps,
                                                        float* __restrict__ ws) {
    extern __shared__ float sm_lds[];
    const int li = sm_find(prefix, n_labels, blockIdx.x);
    const SmLabel L = labels[li];
    const int t = blockIdx.x - prefix[li];
    const int xchunks = (L.dx + 63) / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = (t / xchunks) * 4 + wave;                   // row of the box: z * dy + y
    const int xc = (t % xchunks) * 64;
    const int seg = 64 + 2 * L.r;
    float* s = sm_lds + wave * seg;
    const bool live = row < L.dz * L.dy;
    if (live) {
        const int z = L.z0 + row / L.dy, y = row % L.dy;
        const bool s2 = z >= segs.first[2], s1 = z >= segs.first[1];
        const void* base = s2 ? segs.base[2] : (s1 ? segs.base[1] : segs.base[0]);
        const int zl = z - (s2 ? segs.first[2] : (s1 ? segs.first[1] : segs.first[0]));
        const T* p = (const T*)base + ((int64_t)zl * H + (L.y0 + y)) * W + L.x0;
        for (int i = lane; i < seg; i += 64) {
            const int x = xc - L.r + i;
            s[i] = (x >= 0 && x < L.dx && (uint32_t)p[x] == L.label) ? 1.0f : 0.0f;
        }
    }
    __syncthreads();
    if (!live || xc + lane >= L.dx) return;
    const float* tp = taps + L.tap_off;
    float acc = 0.0f;
    for (int k = 0; k <= 2 * L.r; ++k) acc = fmaf(tp[k], s[lane + k], acc);
    ws[L.ws_off + (int64_t)row * L.dx + xc + lane] = acc;
}

// 1-D convolution along y (AXIS 0: T1 -> T2) or z (AXIS 1: T2 -> field -> threshold / dense float output).
// Block = SM_TL outputs along the axis x SM_TX columns of one (outer) plane; thread = one column, SM_OPT consecutive outputs.
// AXIS 1 writes the planes own[li] = {first (box-local), how many} of the box only, into an output whose plane 0 is the volume's plane
// own0: a z-chunk's own planes, or {0, dz} and 0 for a whole volume.  The inputs are the box's planes [0, dz) whatever is written.
template <int AXIS, bool FLOAT_OUT>
__global__ __launch_bounds__(256) void sm_conv_axis_kernel(const SmLabel* __restrict__ labels, const int* __restrict__ prefix, int n_labels,
                                                           const int2* __restrict__ own, int own0, const float* __restrict__ taps,
                                                           float* __restrict__ ws, int H, int W, uint32_t* __restrict__ winner,
                                                           float* __restrict__ dense) {
    extern __shared__ float sm_lds[];
    const int li = sm_find(prefix, n_labels, blockIdx.x);
    const SmLabel L = labels[li];
    int t = blockIdx.x - prefix[li];
    const int len = AXIS == 0 ? L.dy : L.dz;                    // convolved axis: inputs [0, len)
    int lbeg = 0, lend = len;                                   // outputs [lbeg, lend)
    if (AXIS == 1) { const int2 O = own[li]; lbeg = O.x; lend = O.x + O.y; }
    const int64_t st_axis = AXIS == 0 ? L.dx : (int64_t)L.dy * L.dx;
    const int64_t st_outer = AXIS == 0 ? (int64_t)L.dy * L.dx : L.dx;
    const int xchunks = (L.dx + SM_TX - 1) / SM_TX, lchunks = (lend - lbeg + SM_TL - 1) / SM_TL;
    const int xc = (t % xchunks) * SM_TX; t /= xchunks;
    const int l0 = lbeg + (t % lchunks) * SM_TL;
    const int outer = t / lchunks;
    const int64_t vol = (int64_t)L.dz * L.dy * L.dx;
    const float* src = ws + L.ws_off + (AXIS == 0 ? 0 : vol) + outer * st_outer;
    const int rows = SM_TL + 2 * L.r;
    const int xl = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const bool xok = xc + xl < L.dx;
    for (int j = grp; j < rows; j += 4) {
        const int l = l0 - L.r + j;
        sm_lds[j * SM_TX + xl] = (xok && l >= 0 && l < len) ? src[l * st_axis + xc + xl] : 0.0f;
    }
    __syncthreads();
    const int o0 = grp * SM_OPT;                                // this thread's outputs l0 + o0 .. + SM_OPT-1
    if (!xok || l0 + o0 >= lend) return;
    // input j (relative to l0 + o0 - r) feeds output o with tap j - o; the tap table has SM_OPT-1 zeros on both sides
    const float* tp = taps + L.tap_off;
    float acc[SM_OPT];
#pragma unroll
    for (int o = 0; o < SM_OPT; ++o) acc[o] = 0.0f;
    const float* col = sm_lds + o0 * SM_TX + xl;
    for (int j = 0; j < 2 * L.r + SM_OPT; ++j) {
        const float v = col[j * SM_TX];
#pragma unroll
        for (int o = 0; o < SM_OPT; ++o) acc[o] = fmaf(tp[j - o], v, acc[o]);
    }
#pragma unroll
    for (int o = 0; o < SM_OPT; ++o) {
        const int l = l0 + o0 + o;
        if (l >= lend) break;
        if (AXIS == 0) {
            ws[L.ws_off + vol + outer * st_outer + l * st_axis + xc + xl] = acc[o];
        } else {
            const int64_t g = ((int64_t)(L.z0 + l - own0) * H + (L.y0 + outer)) * W + L.x0 + xc + xl;
            if (FLOAT_OUT) dense[g] = acc[o];
            else if (acc[o] > 0.5f) atomicMax(winner + g, L.label);
        }
    }
}

__global__ __launch_bounds__(256) void sm_cast_kernel(const uint32_t* __restrict__ winner, uint8_t* __restrict__ out, int64_t n) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const uint4 w = reinterpret_cast<const uint4*>(winner)[i];
        reinterpret_cast<uint32_t*>(out)[i] = (w.x & 255u) | ((w.y & 255u) << 8) | ((w.z & 255u) << 16) | (w.w << 24);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) out[(n4 << 2) + threadIdx.x] = (uint8_t)winner[(n4 << 2) + threadIdx.x];
}

// counts[v] = stats[v].count as int64 (saber_label_counts)
__global__ __launch_bounds__(256) void sm_counts_kernel(const uint32_t* __restrict__ stats, int n, int64_t* __restrict__ counts) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < n) counts[v] = (int64_t)stats[(size_t)v * 8];
}

// kernel size and taps exactly as gaussian.py:97-104 computes them (float32 taps, float32 normalisation)
static int sm_kernel_size(double sigma) {
    int ks = (int)(2 * 3 * sigma + 1);
    if (ks % 2 == 0) ks += 1;
    return ks;
}
// sigma of a label of `count` voxels: scale * the diameter of the sphere of that volume (masks.py:303-308)
static double sm_label_sigma(double count, double scale) {
    const double approx_diameter = 2.0 * std::pow((3.0 * count) / (4.0 * M_PI), 1.0 / 3.0);
    return scale * approx_diameter;
}
static int sm_make_taps(double sigma, std::vector<float>& out) {
    const int ks = sm_kernel_size(sigma);
    const int r = ks / 2;
    const float den = (float)(2.0 * sigma * sigma);
    std::vector<float> t(ks);
    float sum = 0.0f;
    for (int i = -r; i <= r; ++i) { t[i + r] = expf(-(float)(i * i) / den); sum += t[i + r]; }
    for (int i = 0; i < ks; ++i) out.push_back(t[i] / sum);
    return r;
}

#define SM_MAX_LABEL (1u << 22)
#define SM_LDS_LIMIT (150 * 1024)

namespace {
struct SmScratch {
    uint32_t* winner = nullptr;
    SmLabel* labels = nullptr;
    int2* own = nullptr;
    int* prefix = nullptr;
    float *taps = nullptr, *ws = nullptr;
    void release() {
        (void)hipFree(winner); (void)hipFree(labels); (void)hipFree(own); (void)hipFree(prefix); (void)hipFree(taps); (void)hipFree(ws);
    }
};

// f(T()) with T the unsigned type of elem_bytes (1, 2 or 4) bytes
template <typename F>
void sm_by_elem(int elem_bytes, F&& f) {
    if (elem_bytes == 1) f(uint8_t());
    else if (elem_bytes == 2) f(uint16_t());
    else f(uint32_t());
}

// largest label value (atomicMax into *out) and stats[v] of a label volume; with zflag only the planes z whose zflag[z] is set count.
// They only enqueue.
void sm_launch_max(const void* lab, int elem_bytes, const uint8_t* zflag, int64_t plane, int64_t n, uint32_t* out, hipStream_t s) {
    sm_by_elem(elem_bytes, [&](auto t) {
        using T = decltype(t);
        if (zflag) hipLaunchKernelGGL((sm_max_kernel<T, true>), dim3(eng_blocks(n)), dim3(256), 0, s, (const T*)lab, zflag, plane, n, out);
        else hipLaunchKernelGGL((sm_max_kernel<T, false>), dim3(eng_blocks(n)), dim3(256), 0, s, (const T*)lab, zflag, plane, n, out);
    });
}
void sm_launch_stats(const void* lab, int elem_bytes, const uint8_t* zflag, int Z, int H, int W, uint32_t* stats, hipStream_t s) {
    const int64_t rows = (int64_t)Z * H;
    const unsigned grid = (unsigned)((rows * ((W + 511) / 512) + 3) / 4);
    sm_by_elem(elem_bytes, [&](auto t) {
        using T = decltype(t);
        if (zflag) hipLaunchKernelGGL((sm_stats_kernel<T, true>), dim3(grid), dim3(256), 0, s, (const T*)lab, zflag, W, rows, H, stats);
        else hipLaunchKernelGGL((sm_stats_kernel<T, false>), dim3(grid), dim3(256), 0, s, (const T*)lab, zflag, W, rows, H, stats);
    });
}
}  // namespace

hipError_t label_max_host(const void* const* bufs, const int64_t* n, int n_bufs, int elem_bytes, const uint8_t* zflag, int64_t plane,
                          uint32_t* out_max, hipStream_t s) {
    uint32_t* dev = nullptr;
    hipError_t st = hipMalloc(&dev, 4);
    if (st == hipSuccess) st = hipMemsetAsync(dev, 0, 4, s);
    if (st == hipSuccess) {
        for (int b = 0; b < n_bufs; ++b)
            if (n[b]) sm_launch_max(bufs[b], elem_bytes, zflag, plane, n[b], dev, s);
        st = hipGetLastError();
    }
    if (st == hipSuccess) st = hipMemcpyAsync(out_max, dev, 4, hipMemcpyDeviceToHost, s);
    if (st == hipSuccess) st = hipStreamSynchronize(s);
    (void)hipFree(dev);
    return st;
}

hipError_t label_stats_host(const void* const* bufs, const int* planes, int n_bufs, int elem_bytes, const uint8_t* zflag, int H, int W,
                            size_t n_stats, std::vector<uint32_t>& st, hipStream_t s) {
    const size_t rows = (size_t)n_bufs * n_stats;
    st.resize(rows * 8);
    for (size_t v = 0; v < rows; ++v) { uint32_t* p = &st[v * 8]; p[0] = 0; p[1] = p[2] = p[3] = 0xffffffffu; p[4] = p[5] = p[6] = p[7] = 0; }
    uint32_t* dev = nullptr;
    hipError_t err = hipMalloc(&dev, rows * 32);
    if (err == hipSuccess) err = hipMemcpyAsync(dev, st.data(), rows * 32, hipMemcpyHostToDevice, s);
    if (err == hipSuccess) {
        for (int b = 0; b < n_bufs; ++b)
            if (planes[b]) sm_launch_stats(bufs[b], elem_bytes, zflag, planes[b], H, W, dev + (size_t)b * n_stats * 8, s);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(st.data(), dev, rows * 32, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    (void)hipFree(dev);
    return err;
}

// Steps 3-6 for the labels of `labs` (ascending label value; their ws_off is set here): the volume's planes are read through `segs`,
// label i writes the planes owns[i] of its box, and plane own0 of the volume is plane 0 of the output - the uint8 label volume out_u8 of
// n_out voxels (through a winner volume of its own), or the dense float field of the one label.  Labels run in groups whose two fp32
// boxes fit the workspace (>= the largest single label, at least 1 GiB of floats when useful); one host synchronisation per group.
static int sm_convolve(saber_engine* e, const char* who, const SmSegs& segs, int elem_bytes, int H, int W, std::vector<SmLabel>& labs,
                       const std::vector<int2>& owns, int own0, const std::vector<float>& taps, uint8_t* out_u8, int64_t n_out, float* out_dense,
                       hipStream_t s) {
    SmScratch S;
    auto cleanup = [&]() { S.release(); };
    if (labs.empty()) { ENG_HIP(e, hipStreamSynchronize(s)); return SABER_OK; }
    int64_t total = 0, biggest = 0;
    for (auto& L : labs) {
        const int64_t v = (int64_t)L.dz * L.dy * L.dx;
        total += 2 * v;
        biggest = std::max(biggest, v);
    }
    const int64_t ws_floats = std::min(total, std::max<int64_t>(2 * biggest, (int64_t)1 << 28));
    const size_t stride = labs.size() + 1;
    ENG_HIP_CLEANUP(e, hipMalloc(&S.ws, (size_t)ws_floats * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&S.taps, taps.size() * 4));
    ENG_HIP_CLEANUP(e, hipMemcpyAsync(S.taps, taps.data(), taps.size() * 4, hipMemcpyHostToDevice, s));
    ENG_HIP_CLEANUP(e, hipMalloc(&S.labels, labs.size() * sizeof(SmLabel)));
    ENG_HIP_CLEANUP(e, hipMalloc(&S.own, labs.size() * sizeof(int2)));
    ENG_HIP_CLEANUP(e, hipMalloc(&S.prefix, 3 * stride * sizeof(int)));
    if (out_u8) {
        ENG_HIP_CLEANUP(e, hipMalloc(&S.winner, (size_t)n_out * 4));
        ENG_HIP_CLEANUP(e, hipMemsetAsync(S.winner, 0, (size_t)n_out * 4, s));
    }
    ENG_HIP_CLEANUP(e, hipFuncSetAttribute((const void*)sm_conv_axis_kernel<0, false>, hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_LIMIT));
    ENG_HIP_CLEANUP(e, hipFuncSetAttribute((const void*)sm_conv_axis_kernel<1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_LIMIT));
    ENG_HIP_CLEANUP(e, hipFuncSetAttribute((const void*)sm_conv_axis_kernel<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_LIMIT));
    std::vector<int> prefix;
    size_t g0 = 0;
    while (g0 < labs.size()) {
        size_t g1 = g0;
        int64_t used = 0;
        int grmax = 0;
        int64_t tiles[3] = {0, 0, 0};
        prefix.assign(3 * stride, 0);
        while (g1 < labs.size()) {
            SmLabel& L = labs[g1];
            const int64_t v2 = 2 * (int64_t)L.dz * L.dy * L.dx;
            if (g1 > g0 && used + v2 > ws_floats) break;
            const int64_t xch = (L.dx + 63) / 64;
            const int64_t tx = (((int64_t)L.dz * L.dy + 3) / 4) * xch;
            const int64_t ty = (int64_t)L.dz * ((L.dy + SM_TL - 1) / SM_TL) * xch;
            const int64_t tz = (int64_t)L.dy * ((owns[g1].y + SM_TL - 1) / SM_TL) * xch;
            if (tiles[0] + tx > 0x7fffffff || tiles[1] + ty > 0x7fffffff || tiles[2] + tz > 0x7fffffff) {
                if (g1 == g0) { cleanup(); return eng_fail(e, SABER_ERR_INVALID, std::string(who) + ": label too large"); }
                break;
            }
            L.ws_off = used;
            used += v2;
            grmax = std::max(grmax, L.r);
            const size_t i = g1 - g0;
            prefix[0 * stride + i] = (int)tiles[0]; prefix[1 * stride + i] = (int)tiles[1]; prefix[2 * stride + i] = (int)tiles[2];
            tiles[0] += tx; tiles[1] += ty; tiles[2] += tz;
            ++g1;
        }
        const int ng = (int)(g1 - g0);
        for (int a = 0; a < 3; ++a) prefix[a * stride + ng] = (int)tiles[a];
        ENG_HIP_CLEANUP(e, hipMemcpyAsync(S.labels, labs.data() + g0, (size_t)ng * sizeof(SmLabel), hipMemcpyHostToDevice, s));
        ENG_HIP_CLEANUP(e, hipMemcpyAsync(S.own, owns.data() + g0, (size_t)ng * sizeof(int2), hipMemcpyHostToDevice, s));
        ENG_HIP_CLEANUP(e, hipMemcpyAsync(S.prefix, prefix.data(), prefix.size() * sizeof(int), hipMemcpyHostToDevice, s));
        sm_by_elem(elem_bytes, [&](auto t) {
            hipLaunchKernelGGL(sm_conv_x_kernel<decltype(t)>, dim3((unsigned)tiles[0]), dim3(256), (size_t)4 * (64 + 2 * grmax) * sizeof(float), s, segs,
                               H, W, (const SmLabel*)S.labels, (const int*)S.prefix, ng, (const float*)S.taps, S.ws);
        });
        const size_t lds = (size_t)(SM_TL + 2 * grmax) * SM_TX * sizeof(float);
        hipLaunchKernelGGL((sm_conv_axis_kernel<0, false>), dim3((unsigned)tiles[1]), dim3(256), lds, s, (const SmLabel*)S.labels,
                           (const int*)(S.prefix + stride), ng, (const int2*)S.own, own0, (const float*)S.taps, S.ws, H, W, (uint32_t*)nullptr,
                           (float*)nullptr);
        if (out_u8)
            hipLaunchKernelGGL((sm_conv_axis_kernel<1, false>), dim3((unsigned)tiles[2]), dim3(256), lds, s, (const SmLabel*)S.labels,
                               (const int*)(S.prefix + 2 * stride), ng, (const int2*)S.own, own0, (const float*)S.taps, S.ws, H, W, S.winner,
                               (float*)nullptr);
        else
            hipLaunchKernelGGL((sm_conv_axis_kernel<1, true>), dim3((unsigned)tiles[2]), dim3(256), lds, s, (const SmLabel*)S.labels,
                               (const int*)(S.prefix + 2 * stride), ng, (const int2*)S.own, own0, (const float*)S.taps, S.ws, H, W,
                               (uint32_t*)nullptr, out_dense);
        ENG_HIP_CLEANUP(e, hipGetLastError());
        ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));                    // the descriptor / prefix host buffers are reused by the next group
        g0 = g1;
    }
    if (out_u8) {
        hipLaunchKernelGGL(sm_cast_kernel, dim3((unsigned)std::min<int64_t>((n_out / 4 + 255) / 256 + 1, 1 << 16)), dim3(256), 0, s,
                           (const uint32_t*)S.winner, out_u8, n_out);
        ENG_HIP_CLEANUP(e, hipGetLastError());
    }
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
    cleanup();
    return SABER_OK;
}

// mode 0: label volume -> uint8 (fast_3d_gaussian_smoothing);  mode 1: binary mask (any non-zero) + fixed sigma -> float field.
// The whole volume is the chunk without halos whose own planes are all of them: one segment, every box written on [0, dz), own0 = 0.
static int sm_run(saber_engine* e, const void* vol_dev, int elem_bytes, int Z, int H, int W, double scale, double fixed_sigma, int mode,
                  void* out_dev, int* out_n_labels, hipStream_t s) {
    const int64_t n = (int64_t)Z * H * W;
    ENG_DEVICE(e);
    if (out_n_labels) *out_n_labels = 0;
    uint32_t maxv = 0;
    ENG_HIP(e, label_max_host(&vol_dev, &n, 1, elem_bytes, nullptr, 0, &maxv, s));
    ENG_HIP(e, hipMemsetAsync(out_dev, 0, (size_t)n * (mode == 0 ? 1 : 4), s));
    if (maxv == 0) { ENG_HIP(e, hipStreamSynchronize(s)); return SABER_OK; }
    if (maxv > SM_MAX_LABEL) return eng_fail(e, SABER_ERR_INVALID, "smooth_labels: label values above 2^22 are not supported");
    // ---- per-label count + bounding box
    const size_t n_stats = (size_t)maxv + 1;
    std::vector<uint32_t> st;
    ENG_HIP(e, label_stats_host(&vol_dev, &Z, 1, elem_bytes, nullptr, H, W, n_stats, st, s));
    // ---- host: sigma, radius, taps per present label, ascending label value (np.unique order, masks.py:253-262)
    std::vector<SmLabel> labs;
    std::vector<int2> owns;
    std::vector<float> taps(SM_OPT - 1, 0.0f);
    int rmax = 0;
    for (size_t v = 1; v < n_stats; ++v) {
        const uint32_t* p = &st[v * 8];
        if (!p[0]) continue;
        if (mode == 1 && v != 1) return eng_fail(e, SABER_ERR_INVALID, "gaussian_smoothing_3d: the input must be a 0/1 mask");
        SmLabel L;
        L.label = (uint32_t)v;
        L.z0 = (int)p[1]; L.y0 = (int)p[2]; L.x0 = (int)p[3];
        L.dz = (int)(p[4] - p[1]) + 1; L.dy = (int)(p[5] - p[2]) + 1; L.dx = (int)(p[6] - p[3]) + 1;
        if (mode == 1) { L.z0 = L.y0 = L.x0 = 0; L.dz = Z; L.dy = H; L.dx = W; }      // the float field is wanted everywhere
        double sigma = fixed_sigma;
        if (mode == 0) sigma = sm_label_sigma((double)p[0], scale);
        L.tap_off = (int)taps.size();
        L.r = sm_make_taps(sigma, taps);
        taps.insert(taps.end(), SM_OPT - 1, 0.0f);
        L.ws_off = 0;
        rmax = std::max(rmax, L.r);
        labs.push_back(L);
        owns.push_back(make_int2(0, L.dz));
    }
    if ((size_t)(SM_TL + 2 * rmax) * SM_TX * sizeof(float) > SM_LDS_LIMIT)
        return eng_fail(e, SABER_ERR_INVALID, "smooth_labels: Gaussian radius " + std::to_string(rmax) + " exceeds the supported 284 voxels");
    if (out_n_labels) *out_n_labels = (int)labs.size();
    const SmSegs segs = {{vol_dev, vol_dev, vol_dev}, {0, INT_MAX, INT_MAX}};
    return sm_convolve(e, "smooth_labels", segs, elem_bytes, H, W, labs, owns, 0, taps, mode == 0 ? (uint8_t*)out_dev : nullptr, n,
                       mode == 0 ? nullptr : (float*)out_dev, s);
}

extern "C" int saber_smooth_labels(saber_engine* e, const void* labels_dev, int elem_bytes, int Z, int H, int W, double scale,
                                   uint8_t* out_dev, int* out_n_labels, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!labels_dev || !out_dev || Z <= 0 || H <= 0 || W <= 0 || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) || !(scale > 0.0))
        return eng_fail(e, SABER_ERR_INVALID, "smooth_labels: bad argument");
    if ((int64_t)Z * H * W >= (int64_t)0x7fffffff) return eng_fail(e, SABER_ERR_INVALID, "smooth_labels: volumes of 2^31 voxels or more are not supported");
    return sm_run(e, labels_dev, elem_bytes, Z, H, W, scale, 0.0, 0, out_dev, out_n_labels, (hipStream_t)stream);
}

extern "C" int saber_gaussian_smoothing_3d(saber_engine* e, const uint8_t* mask_dev, int Z, int H, int W, double sigma, float* out_dev,
                                           void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!mask_dev || !out_dev || Z <= 0 || H <= 0 || W <= 0 || !(sigma > 0.0)) return eng_fail(e, SABER_ERR_INVALID, "gaussian_smoothing_3d: bad argument");
    if ((int64_t)Z * H * W >= (int64_t)0x7fffffff) return eng_fail(e, SABER_ERR_INVALID, "gaussian_smoothing_3d: volumes of 2^31 voxels or more are not supported");
    return sm_run(e, mask_dev, 1, Z, H, W, 0.0, sigma, 1, out_dev, nullptr, (hipStream_t)stream);
}

// ---- one z-chunk with its halos (header: saber_smooth_labels_chunk).  Why the own planes come out as the whole volume's: a label's
// field on plane z depends on the planes z - r .. z + r only, all of which lie in the three buffers (halo >= r, or the volume ends);
// sigma and taps come from the whole volume's count; every output sums its taps in ascending order with fma, and a larger box only
// adds terms that are exactly +0.  The box here is the label's box inside the planes [own0 - r, own1 + r): outside it, on an own
// plane, only one side of the kernel can meet the part of the mask that reaches that plane, so the field stays below 0.5 there, as
// outside the whole volume's box.  A label whose voxels in those planes all lie below (or all above) the own planes has an empty
// range of own planes inside its box and is skipped; one with voxels on both sides and none between (a "sandwich") is not.
extern "C" int saber_smooth_radius(int64_t count, double scale, int* out_radius) {
    if (!out_radius || count < 0 || !(scale > 0.0)) return SABER_ERR_INVALID;
    *out_radius = count ? sm_kernel_size(sm_label_sigma((double)count, scale)) / 2 : 0;
    return SABER_OK;
}

extern "C" int saber_smooth_labels_chunk(saber_engine* e, const void* lo_dev, int lo_planes, const void* own_dev, int own_planes,
                                         const void* hi_dev, int hi_planes, int lo_is_volume_end, int hi_is_volume_end, int elem_bytes, int H,
                                         int W, const uint32_t* ids_host, const int64_t* counts_host, int n_ids, double scale,
                                         uint8_t* out_dev, int* out_n_labels, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!own_dev || !out_dev || own_planes <= 0 || lo_planes < 0 || hi_planes < 0 || (lo_planes && !lo_dev) || (hi_planes && !hi_dev) || H <= 0 ||
        W <= 0 || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) || !(scale > 0.0) || n_ids < 0 || (n_ids && (!ids_host || !counts_host)))
        return eng_fail(e, SABER_ERR_INVALID, "smooth_labels_chunk: bad argument");
    const int64_t E = (int64_t)lo_planes + own_planes + hi_planes;
    if (E * H * W >= (int64_t)0x7fffffff)
        return eng_fail(e, SABER_ERR_INVALID, "smooth_labels_chunk: 2^31 - 1 voxels or more over the three buffers are not supported");
    hipStream_t s = (hipStream_t)stream;
    const int own0 = lo_planes, own1 = lo_planes + own_planes;
    const int64_t plane = (int64_t)H * W, n_own = (int64_t)own_planes * plane;
    // ---- the table: ascending label values, positive counts; its largest radius is what the halos must hold
    std::vector<int> radius(n_ids);
    int rtab = 0;
    for (int i = 0; i < n_ids; ++i) {
        if (ids_host[i] == 0 || ids_host[i] > SM_MAX_LABEL || (i && ids_host[i] <= ids_host[i - 1]) || counts_host[i] <= 0)
            return eng_fail(e, SABER_ERR_INVALID, ids_host[i] > SM_MAX_LABEL ? "smooth_labels_chunk: label values above 2^22 are not supported"
                                                                            : "smooth_labels_chunk: the table must list ascending label values > 0 with counts > 0");
        radius[i] = sm_kernel_size(sm_label_sigma((double)counts_host[i], scale)) / 2;
        rtab = std::max(rtab, radius[i]);
    }
    if ((size_t)(SM_TL + 2 * rtab) * SM_TX * sizeof(float) > SM_LDS_LIMIT)
        return eng_fail(e, SABER_ERR_INVALID, "smooth_labels_chunk: Gaussian radius " + std::to_string(rtab) + " exceeds the supported 284 voxels");
    if ((lo_planes < rtab && !lo_is_volume_end) || (hi_planes < rtab && !hi_is_volume_end))
        return eng_fail(e, SABER_ERR_INVALID, "smooth_labels_chunk: a halo of " + std::to_string(lo_planes < rtab && !lo_is_volume_end ? lo_planes : hi_planes) +
                                                  " planes is shorter than the largest radius " + std::to_string(rtab) + " and is not the volume's end");
    ENG_DEVICE(e);
    if (out_n_labels) *out_n_labels = 0;
    const void* bufs[3] = {lo_dev, own_dev, hi_dev};
    const int planes[3] = {lo_planes, own_planes, hi_planes};
    const int64_t voxels[3] = {lo_planes * plane, n_own, hi_planes * plane};
    const int first[3] = {0, own0, own1};
    uint32_t maxv = 0;
    ENG_HIP(e, label_max_host(bufs, voxels, 3, elem_bytes, nullptr, 0, &maxv, s));
    ENG_HIP(e, hipMemsetAsync(out_dev, 0, (size_t)n_own, s));
    if (maxv == 0) { ENG_HIP(e, hipStreamSynchronize(s)); return SABER_OK; }
    if (maxv > SM_MAX_LABEL) return eng_fail(e, SABER_ERR_INVALID, "smooth_labels_chunk: label values above 2^22 are not supported");
    // ---- count + bounding box per label value and buffer (z local to the buffer)
    const size_t n_stats = (size_t)maxv + 1;
    std::vector<uint32_t> st;
    ENG_HIP(e, label_stats_host(bufs, planes, 3, elem_bytes, nullptr, H, W, n_stats, st, s));
    // ---- host: per label value the box inside [own0 - r, own1 + r) and its own planes, ascending label value
    std::vector<SmLabel> labs;
    std::vector<int2> owns;
    std::vector<float> taps(SM_OPT - 1, 0.0f);
    int ti = 0;
    for (size_t v = 1; v < n_stats; ++v) {
        const uint32_t* q[3] = {&st[v * 8], &st[(n_stats + v) * 8], &st[(2 * n_stats + v) * 8]};
        if (!q[0][0] && !q[1][0] && !q[2][0]) continue;
        while (ti < n_ids && ids_host[ti] < v) ++ti;
        if (ti == n_ids || ids_host[ti] != v)
            return eng_fail(e, SABER_ERR_INVALID, "smooth_labels_chunk: label value " + std::to_string(v) + " is not in the table");
        const int r = radius[ti];
        const int w0 = std::max(0, own0 - r), w1 = (int)std::min<int64_t>(E, (int64_t)own1 + r);       // the planes this label is read on
        // per buffer: present inside the window?  (segment planes; the lower halo lies below w1, the upper one above w0)
        const bool in_lo = q[0][0] && (int)q[0][4] + first[0] >= w0;
        const bool in_own = q[1][0] != 0;
        const bool in_hi = q[2][0] && (int)q[2][1] + first[2] < w1;
        if (!in_own && !(in_lo && in_hi)) continue;                 // all on one side of the own planes, or further than r: skipped
        const bool in[3] = {in_lo, in_own, in_hi};
        int zlo = 0x7fffffff, zhi = -1, ylo = 0x7fffffff, yhi = -1, xlo = 0x7fffffff, xhi = -1;
        for (int b = 0; b < 3; ++b) {
            if (!in[b]) continue;
            zlo = std::min(zlo, (int)q[b][1] + first[b]); zhi = std::max(zhi, (int)q[b][4] + first[b]);
            ylo = std::min(ylo, (int)q[b][2]); yhi = std::max(yhi, (int)q[b][5]);
            xlo = std::min(xlo, (int)q[b][3]); xhi = std::max(xhi, (int)q[b][6]);
        }
        zlo = std::max(zlo, w0); zhi = std::min(zhi, w1 - 1);
        const int o_first = std::max(zlo, own0), o_last = std::min(zhi, own1 - 1);
        if (o_first > o_last) continue;
        zlo = std::max(zlo, o_first - r); zhi = std::min(zhi, o_last + r);      // planes no own output of the box reads
        SmLabel L;
        L.label = (uint32_t)v;
        L.z0 = zlo; L.y0 = ylo; L.x0 = xlo;
        L.dz = zhi - zlo + 1; L.dy = yhi - ylo + 1; L.dx = xhi - xlo + 1;
        L.tap_off = (int)taps.size();
        L.r = sm_make_taps(sm_label_sigma((double)counts_host[ti], scale), taps);
        taps.insert(taps.end(), SM_OPT - 1, 0.0f);
        L.ws_off = 0;
        labs.push_back(L);
        owns.push_back(make_int2(o_first - zlo, o_last - o_first + 1));
    }
    if (out_n_labels) *out_n_labels = (int)labs.size();
    SmSegs segs;
    for (int b = 0; b < 3; ++b) { segs.base[b] = bufs[b]; segs.first[b] = first[b]; }
    return sm_convolve(e, "smooth_labels_chunk", segs, elem_bytes, H, W, labs, owns, own0, taps, out_dev, n_own, nullptr, s);
}

extern "C" int saber_label_max(saber_engine* e, const void* labels_dev, int elem_bytes, int64_t n, uint32_t* out_max, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!labels_dev || !out_max || n <= 0 || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4))
        return eng_fail(e, SABER_ERR_INVALID, "label_max: bad argument");
    ENG_DEVICE(e);
    ENG_HIP(e, label_max_host(&labels_dev, &n, 1, elem_bytes, nullptr, 0, out_max, (hipStream_t)stream));
    return SABER_OK;
}

extern "C" int saber_label_counts(saber_engine* e, const void* labels_dev, int elem_bytes, int Z, int H, int W, int n_counts, int64_t* counts_dev,
                                  void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!labels_dev || !counts_dev || Z <= 0 || H <= 0 || W <= 0 || n_counts <= 0 || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4))
        return eng_fail(e, SABER_ERR_INVALID, "label_counts: bad argument");
    const int64_t n = (int64_t)Z * H * W;
    if (n >= (int64_t)0x7fffffff) return eng_fail(e, SABER_ERR_INVALID, "label_counts: volumes of 2^31 voxels or more are not supported");
    if ((int64_t)n_counts > (int64_t)SM_MAX_LABEL + 1) return eng_fail(e, SABER_ERR_INVALID, "label_counts: label values above 2^22 are not supported");
    hipStream_t s = (hipStream_t)stream;
    ENG_DEVICE(e);
    uint32_t maxv = 0;
    ENG_HIP(e, label_max_host(&labels_dev, &n, 1, elem_bytes, nullptr, 0, &maxv, s));
    if (maxv >= (uint32_t)n_counts)                                  // the statistics kernel indexes its table by label value
        return eng_fail(e, SABER_ERR_INVALID, "label_counts: label value " + std::to_string(maxv) + " does not fit a table of " + std::to_string(n_counts));
    uint32_t* stats = nullptr;
    auto cleanup = [&]() { (void)hipFree(stats); };
    ENG_HIP_CLEANUP(e, hipMalloc(&stats, (size_t)n_counts * 32));
    ENG_HIP_CLEANUP(e, hipMemsetAsync(stats, 0, (size_t)n_counts * 32, s));
    sm_launch_stats(labels_dev, elem_bytes, nullptr, Z, H, W, stats, s);
    hipLaunchKernelGGL(sm_counts_kernel, dim3((unsigned)((n_counts + 255) / 256)), dim3(256), 0, s, (const uint32_t*)stats, n_counts, counts_dev);
    ENG_HIP_CLEANUP(e, hipGetLastError());
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
    cleanup();
    return SABER_OK;
}
