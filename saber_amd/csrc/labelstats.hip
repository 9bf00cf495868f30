// Organelle statistics on the device: per-label integer moments of a (Z,H,W) label volume and what the reference derives from them.
// Replaces the per-label loop of saber.analysis.organelle_statistics.extract_organelle_statistics (saber/analysis/organelle_statistics.py:15-68):
// np.unique (:15-16), `(mask == label).astype(int)` with two np.sum over the whole volume (:22-25, :40) and skimage.measure.regionprops on it
// (:30-31 centroid, :44-45 axis_major_length / axis_minor_length), which is O(K N) host work with K full-volume temporaries.
//
// Everything the reference reports follows from ten integer sums per label, so the volume is read a fixed number of times whatever K is:
//   ls_presence     one read: a bitmap of the label values present (the device's np.unique).  Lanes whose left neighbour holds the same
//                   value stay silent and a set bit is not set again, so the atomic ORs are a few per label and wave, not one per voxel.
//   ls_rank         one block: exclusive prefix sum of the bitmap words' population counts.  rank(v) = rankbase[v >> 5] + popc(bits of
//                   the word below v): the dense table has K rows in ascending label order and nothing is sized by the largest value
//                   (bitmap and rank table are fixed: 2^22 + 1 bits for the 32-bit types, the whole range for the narrow ones).
//   ls_labels       the K label values, from the bitmap.
//   ls_moments      one read: 16 uint64 words per label, LS_WORDS below.  A wave owns a 512-voxel piece of a row (z and y fixed), lane l
//                   holds the voxels l, l + 64, ... (coalesced loads) and sums count, sum d, sum d^2 of the piece-relative offsets d < 512
//                   of its current label in 32-bit registers.  At the end of the piece the lanes that hold the same label combine (the
//                   pattern of sm_stats_kernel, smooth3d.hip); only those three sums and the two x bounds cross lanes.  The ten
//                   sums are those three times z, y, z^2, y^2, zy (64-bit), formed by 16 lanes, one word each, so a table update is one
//                   128-byte row.  The updates go to a table in LDS keyed by the label's rank (128 direct-mapped slots; a rank that finds
//                   its slot taken by another goes to global memory directly) and a block covers up to 64 consecutive pieces, so what
//                   reaches global memory is one 16-word row per block and label instead of one per piece and label.  BLOCK_TABLE =
//                   false is the per-piece global-atomics form, kept as the baseline the LDS form is measured against (mode 1).
//   ls_finalize     one thread per label, fp64: the numerators n M_ab - S_a S_b of the covariance exactly in 128-bit integers (below 2^96
//                   under the limits), one rounding to fp64, / n^2; eigenvalues of the symmetric 3x3 by cyclic Jacobi, 8 sweeps;
//                   axis_major_length = sqrt(20 l_max), axis_minor_length = sqrt(20 max(l_min, 0)) (skimage: sqrt(10 (ev0 + ev1 - ev2)) /
//                   sqrt(10 (-ev0 + ev1 + ev2)) on the eigenvalues of the inertia tensor tr(C) Id - C).
// Only 64-bit integer atomics and plain stores: the table is exact and order-independent, so two calls give the same bits.
// Limits (checked in the C-ABI): Z, H, W <= 65535 and Z H W < 2^31, so every sum stays below 2^63.  Host synchronisations per call: 2
// (the label count; the end of the call), whatever K is.
#include <algorithm>
#include <string>
#include <type_traits>

#include "common.h"
#include "engine.h"

#define LS_WORDS 16              // n, Sz, Sy, Sx, Szz, Syy, Sxx, Szy, Szx, Syx, zmin, ymin, xmin, zmax, ymax, xmax
#define LS_SLOTS 128             // rows of the block's LDS table (16 KiB)
#define LS_VPL 8                 // voxels per lane and piece
#define LS_PIECE (64 * LS_VPL)
#define LS_MAX_PIECES 64         // pieces per block
#define LS_MAX_LABEL (1u << 22)  // MAX_LABEL of analysis/refine_membranes.py
#define LS_EMPTY 0xffffffffu
#define LS_BITMAP_WORDS (((LS_MAX_LABEL >> 5) + 1 + 31) & ~31u)

typedef unsigned long long ls_u64;

// negative values of the signed types are background
template <typename T>
__device__ __forceinline__ uint32_t ls_value(T v) {
    if (std::is_signed<T>::value && v < (T)0) return 0u;
    return (uint32_t)v;
}

__device__ __forceinline__ ls_u64 ls_identity(int j) { return (j >= 10 && j < 13) ? ~0ull : 0ull; }

// word j of a table row: sums add, lower bounds take the minimum, upper bounds the maximum
__device__ __forceinline__ void ls_apply(ls_u64* p, int j, ls_u64 val) {
    if (j < 10) atomicAdd(p, val);
    else if (j < 13) atomicMin(p, val);
    else atomicMax(p, val);
}

// ------------------------------------------------------------------------------------------------ label compaction
template <typename T>
__global__ __launch_bounds__(256) void ls_presence_kernel(const T* __restrict__ lab, int64_t n, uint32_t* bitmap, uint32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * 256;
    uint32_t last = 0u;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += stride) {      // wave-uniform bound: every lane takes part in the shuffle
        const int64_t i = base + threadIdx.x;
        uint32_t v = i < n ? ls_value(lab[i]) : 0u;
        if (sizeof(T) == 4 && v > LS_MAX_LABEL) { *bad = 1u; v = 0u; }               // every writer stores the same value
        const uint32_t left = (uint32_t)__shfl_up((int)v, 1, 64);
        if (v && v != last && (lane == 0 || v != left)) {
            const uint32_t bit = 1u << (v & 31);
            // a read that goes past the L1: a stale line would only cost a redundant atomic
            if (!(__hip_atomic_load(&bitmap[v >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(&bitmap[v >> 5], bit);
        }
        last = v;
    }
}

// one block of 1024 threads: rankbase[w] = set bits in the words below w, counters[0] = K
__global__ __launch_bounds__(1024) void ls_rank_kernel(const uint32_t* __restrict__ bitmap, int nw, uint32_t* __restrict__ rankbase,
                                                       uint32_t* __restrict__ counters) {
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    const int per = (nw + 1023) / 1024;
    const int w0 = min(t * per, nw), w1 = min(w0 + per, nw);
    uint32_t s = 0;
    for (int w = w0; w < w1; ++w) s += (uint32_t)__popc(bitmap[w]);
    part[t] = s;
    block_scan_inclusive<1024>(part, t);
    uint32_t run = part[t] - s;
    for (int w = w0; w < w1; ++w) { rankbase[w] = run; run += (uint32_t)__popc(bitmap[w]); }
    if (t == 1023) counters[0] = part[1023];
}

// the host launches this only when K fits the caller's capacity
__global__ __launch_bounds__(256) void ls_labels_kernel(const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ rankbase, int nw,
                                                        uint32_t* __restrict__ labels) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= nw) return;
    uint32_t m = bitmap[w], r = rankbase[w];
    while (m) {
        labels[r++] = (uint32_t)w * 32u + (uint32_t)(__ffs((int)m) - 1);
        m &= m - 1u;
    }
}

__global__ __launch_bounds__(256) void ls_init_kernel(ls_u64* __restrict__ mom, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) mom[i] = ls_identity((int)(i & 15));
}

// ------------------------------------------------------------------------------------------------ moments
template <typename T, bool BLOCK_TABLE>
__global__ __launch_bounds__(256) void ls_moments_kernel(const T* __restrict__ lab, int W, int H, int64_t rows, int chunks, int pieces_per_block,
                                                         const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ rankbase,
                                                         ls_u64* __restrict__ mom) {
    __shared__ ls_u64 tab[BLOCK_TABLE ? LS_SLOTS * LS_WORDS : 1];
    __shared__ uint32_t tag[BLOCK_TABLE ? LS_SLOTS : 1];
    if (BLOCK_TABLE) {
        for (int i = threadIdx.x; i < LS_SLOTS * LS_WORDS; i += 256) tab[i] = ls_identity(i & 15);
        for (int i = threadIdx.x; i < LS_SLOTS; i += 256) tag[i] = LS_EMPTY;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = rows * chunks;
    const int64_t first = (int64_t)blockIdx.x * pieces_per_block, end = min(first + pieces_per_block, total);
    for (int64_t piece = first + wave; piece < end; piece += 4) {                     // wave-uniform
        const int64_t row = piece / chunks;
        const uint32_t xb = (uint32_t)(piece % chunks) * LS_PIECE;
        const uint32_t z = (uint32_t)(row / H), y = (uint32_t)(row % H);
        const T* p = lab + row * W + xb;
        uint32_t vals[LS_VPL];
        bool some = false;
#pragma unroll
        for (int i = 0; i < LS_VPL; ++i) {
            const uint32_t d = (uint32_t)(i * 64 + lane);
            vals[i] = (xb + d < (uint32_t)W) ? ls_value(p[d]) : 0u;
            if (sizeof(T) == 4 && vals[i] > LS_MAX_LABEL) vals[i] = 0u;
            some = some || vals[i] != 0u;
        }
        if (!__ballot(some)) continue;
        // cur: the label this lane is summing (background voxels in between do not end it); d: offsets from xb
        uint32_t cur = 0, cnt = 0, sd = 0, sdd = 0, lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i <= LS_VPL; ++i) {
            const uint32_t d = (uint32_t)(i * 64 + lane);
            const uint32_t v = i < LS_VPL ? vals[i] : 0u;
            // a lane hands its sums over when another label begins, and at the end of the piece
            uint32_t pend = (i == LS_VPL) ? cur : ((v && cur && v != cur) ? cur : 0u);
            while (true) {
                const uint64_t any = __ballot(pend != 0u);
                if (!any) break;
                const int leader = __ffsll((long long)any) - 1;
                const uint32_t lv = (uint32_t)__shfl((int)pend, leader, 64);
                const bool mine = (pend == lv);
                uint32_t a = mine ? cnt : 0u, b = mine ? sd : 0u, c = mine ? sdd : 0u, l = mine ? lo : 0xffffffffu, h = mine ? hi : 0u;
                for (int o = 32; o > 0; o >>= 1) {
                    a += (uint32_t)__shfl_xor((int)a, o, 64);
                    b += (uint32_t)__shfl_xor((int)b, o, 64);
                    c += (uint32_t)__shfl_xor((int)c, o, 64);
                    l = min(l, (uint32_t)__shfl_xor((int)l, o, 64));
                    h = max(h, (uint32_t)__shfl_xor((int)h, o, 64));
                }
                // every lane holds the totals now.  lv was present in the first pass, so its bit is set; were the volume changed under
                // the call, a value without a bit is dropped, so that a rank always lies inside the table
                const uint32_t word = bitmap[lv >> 5];
                const bool known = (word >> (lv & 31)) & 1u;
                const uint32_t rank = rankbase[lv >> 5] + (uint32_t)__popc(word & ((1u << (lv & 31)) - 1u));
                int in_lds = 0;
                if (BLOCK_TABLE && known) {
                    if (lane == 0) {
                        const uint32_t old = atomicCAS(&tag[rank & (LS_SLOTS - 1)], LS_EMPTY, rank);
                        in_lds = (old == LS_EMPTY || old == rank) ? 1 : 0;
                    }
                    in_lds = __shfl(in_lds, 0, 64);
                }
                if (lane < LS_WORDS && known) {
                    const int j = lane;
                    const ls_u64 C = a, X = xb, zz = z, yy = y;
                    const ls_u64 SX = C * X + b, SXX = C * X * X + 2ull * X * b + c;
                    const ls_u64 val = j == 0 ? C : j == 1 ? C * zz : j == 2 ? C * yy : j == 3 ? SX : j == 4 ? C * zz * zz : j == 5 ? C * yy * yy
                                     : j == 6 ? SXX : j == 7 ? C * zz * yy : j == 8 ? zz * SX : j == 9 ? yy * SX
                                     : (j == 10 || j == 13) ? zz : (j == 11 || j == 14) ? yy : j == 12 ? X + l : X + h;
                    if (BLOCK_TABLE && in_lds) ls_apply(&tab[(rank & (LS_SLOTS - 1)) * LS_WORDS + j], j, val);
                    else ls_apply(&mom[(size_t)rank * LS_WORDS + j], j, val);
                }
                if (mine) pend = 0u;
            }
            if (v && v != cur) { cur = v; cnt = 0; sd = 0; sdd = 0; lo = d; }
            if (v) { ++cnt; sd += d; sdd += d * d; hi = d; }
        }
    }
    if (BLOCK_TABLE) {
        __syncthreads();
        for (int i = threadIdx.x; i < LS_SLOTS * LS_WORDS; i += 256) {
            const uint32_t rank = tag[i >> 4];
            if (rank != LS_EMPTY) ls_apply(&mom[(size_t)rank * LS_WORDS + (i & 15)], i & 15, tab[i]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ finalise
// |v| < 2^127 to fp64 with one rounding: the top 64 bits with a sticky bit, then an exact scaling
__device__ __forceinline__ double ls_i128_to_double(__int128 v) {
    const bool neg = v < 0;
    const unsigned __int128 u = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
    const ls_u64 hi = (ls_u64)(u >> 64), lo = (ls_u64)u;
    double r;
    if (hi == 0ull) r = (double)lo;
    else {
        const int s = 64 - __clzll((long long)hi);              // 1..63
        ls_u64 m = (ls_u64)(u >> s);
        if (lo & ((1ull << s) - 1ull)) m |= 1ull;               // sticky: m keeps 64 significant bits, 11 more than fp64 rounds at
        r = ldexp((double)m, s);
    }
    return neg ? -r : r;
}

// one Jacobi rotation that zeroes apq; r is the third index
__device__ __forceinline__ void ls_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double p = arp, q = arq;
    arp = c * p - s * q;
    arq = s * p + c * q;
}

// stats[k] = cz, cy, cx, axis_major_length, axis_minor_length, l0 >= l1 >= l2 (eigenvalues of the covariance of the voxel coordinates)
__global__ __launch_bounds__(256) void ls_finalize_kernel(const ls_u64* __restrict__ mom, int K, double* __restrict__ stats) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const ls_u64* m = mom + (size_t)k * LS_WORDS;
    const ls_u64 n = m[0], sz = m[1], sy = m[2], sx = m[3];
    const double dn = (double)n, n2 = (double)(n * n);          // n < 2^31
    auto cov = [&](ls_u64 mab, ls_u64 sa, ls_u64 sb) {
        const __int128 num = (__int128)n * (__int128)mab - (__int128)sa * (__int128)sb;
        return ls_i128_to_double(num) / n2;
    };
    double a00 = cov(m[4], sz, sz), a11 = cov(m[5], sy, sy), a22 = cov(m[6], sx, sx);
    double a01 = cov(m[7], sz, sy), a02 = cov(m[8], sz, sx), a12 = cov(m[9], sy, sx);
    for (int sweep = 0; sweep < 8; ++sweep) {
        ls_rotate(a00, a11, a01, a02, a12);
        ls_rotate(a00, a22, a02, a01, a12);
        ls_rotate(a11, a22, a12, a01, a02);
    }
    double l0 = fmax(a00, fmax(a11, a22)), l2 = fmin(a00, fmin(a11, a22));
    double l1 = a00 + a11 + a22 - l0 - l2;
    l1 = fmin(fmax(l1, l2), l0);
    double* o = stats + (size_t)k * 8;
    o[0] = (double)sz / dn; o[1] = (double)sy / dn; o[2] = (double)sx / dn;
    o[3] = sqrt(20.0 * fmax(l0, 0.0));
    o[4] = sqrt(20.0 * fmax(l2, 0.0));                          // no equivalent-sphere fall-back: a flat label has minor length 0
    o[5] = l0; o[6] = l1; o[7] = l2;
}

// ------------------------------------------------------------------------------------------------ host side
namespace {
template <typename T>
void ls_launch(const T* lab, int Z, int H, int W, int mode, uint32_t* bitmap, uint32_t* rankbase, ls_u64* mom, hipStream_t s) {
    const int64_t rows = (int64_t)Z * H;
    const int chunks = (W + LS_PIECE - 1) / LS_PIECE;
    const int64_t total = rows * chunks;
    // up to 64 pieces per block, fewer on a small volume so that the grid still fills the device
    const int ppb = (int)std::max<int64_t>(4, std::min<int64_t>(LS_MAX_PIECES, (total / 2048) & ~(int64_t)3));
    const unsigned grid = (unsigned)((total + ppb - 1) / ppb);
    if (mode == 0) hipLaunchKernelGGL((ls_moments_kernel<T, true>), dim3(grid), dim3(256), 0, s, lab, W, H, rows, chunks, ppb, (const uint32_t*)bitmap,
                                      (const uint32_t*)rankbase, mom);
    else hipLaunchKernelGGL((ls_moments_kernel<T, false>), dim3(grid), dim3(256), 0, s, lab, W, H, rows, chunks, ppb, (const uint32_t*)bitmap,
                            (const uint32_t*)rankbase, mom);
}

template <typename T>
int ls_run(saber_engine* e, const T* lab, int Z, int H, int W, int capacity, int mode, uint32_t* labels_out, ls_u64* mom, double* stats,
           int* out_n_labels, hipStream_t s) {
    const int64_t n = (int64_t)Z * H * W;
    ENG_DEVICE(e);
    if (!e->labelstats_ws) {
        void* p = nullptr;
        const int st = eng_alloc_bytes(e, &p, (2 * (size_t)LS_BITMAP_WORDS + 4) * sizeof(uint32_t));
        if (st != SABER_OK) return st;
        e->labelstats_ws = p;
    }
    uint32_t* bitmap = (uint32_t*)e->labelstats_ws;
    uint32_t* rankbase = bitmap + LS_BITMAP_WORDS;
    uint32_t* counters = rankbase + LS_BITMAP_WORDS;            // [0] K, [1] a 32-bit value above 2^22 was seen
    const uint32_t vmax = sizeof(T) == 4 ? LS_MAX_LABEL : (sizeof(T) == 2 ? (std::is_signed<T>::value ? 0x7fffu : 0xffffu) : 0xffu);
    const int nw = (int)(vmax >> 5) + 1;
    ENG_HIP(e, hipMemsetAsync(bitmap, 0, (size_t)nw * 4, s));
    ENG_HIP(e, hipMemsetAsync(counters, 0, 16, s));
    hipLaunchKernelGGL(ls_presence_kernel<T>, dim3(eng_blocks(n)), dim3(256), 0, s, lab, n, bitmap, counters + 1);
    hipLaunchKernelGGL(ls_rank_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t*)bitmap, nw, rankbase, counters);
    ENG_HIP(e, hipGetLastError());
    uint32_t host[2] = {0, 0};
    ENG_HIP(e, hipMemcpyAsync(host, counters, 8, hipMemcpyDeviceToHost, s));
    ENG_HIP(e, hipStreamSynchronize(s));                        // synchronisation 1
    if (host[1]) return eng_fail(e, SABER_ERR_INVALID, "label_statistics: label values above 2^22 are not supported");
    const int64_t K = host[0];
    if (out_n_labels) *out_n_labels = (int)K;
    if (K == 0) return SABER_OK;
    if (K > capacity)
        return eng_fail(e, SABER_ERR_CAPACITY, "label_statistics: the volume holds " + std::to_string(K) + " labels, the output tables have room for " +
                                                   std::to_string(capacity));
    if (!labels_out || !mom || !stats) return eng_fail(e, SABER_ERR_INVALID, "label_statistics: bad argument");
    hipLaunchKernelGGL(ls_labels_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, (const uint32_t*)bitmap, (const uint32_t*)rankbase, nw, labels_out);
    hipLaunchKernelGGL(ls_init_kernel, dim3(eng_blocks(K * LS_WORDS)), dim3(256), 0, s, mom, K * LS_WORDS);
    ls_launch<T>(lab, Z, H, W, mode, bitmap, rankbase, mom, s);
    hipLaunchKernelGGL(ls_finalize_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, (const ls_u64*)mom, (int)K, stats);
    ENG_HIP(e, hipGetLastError());
    ENG_HIP(e, hipStreamSynchronize(s));                        // synchronisation 2
    return SABER_OK;
}
}  // namespace

extern "C" int saber_label_statistics(saber_engine* e, const void* labels_dev, int elem_bytes, int is_signed, int Z, int H, int W, int capacity,
                                      int mode, uint32_t* labels_out_dev, uint64_t* moments_out_dev, double* stats_out_dev, int* out_n_labels,
                                      void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (out_n_labels) *out_n_labels = 0;
    if (!labels_dev || Z <= 0 || H <= 0 || W <= 0 || capacity < 0) return eng_fail(e, SABER_ERR_INVALID, "label_statistics: bad argument");
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return eng_fail(e, SABER_ERR_INVALID, "label_statistics: elem_bytes must be 1, 2 or 4");
    if (elem_bytes == 1 && is_signed) return eng_fail(e, SABER_ERR_INVALID, "label_statistics: 8-bit labels are unsigned");
    if (mode != 0 && mode != 1) return eng_fail(e, SABER_ERR_INVALID, "label_statistics: mode must be 0 (block tables) or 1 (per-piece global atomics)");
    if (Z > 65535 || H > 65535 || W > 65535) return eng_fail(e, SABER_ERR_INVALID, "label_statistics: Z, H and W must not exceed 65535");
    if ((int64_t)Z * H * W >= (int64_t)0x7fffffff) return eng_fail(e, SABER_ERR_INVALID, "label_statistics: volumes of 2^31 voxels or more are not supported");
    hipStream_t s = (hipStream_t)stream;
    ls_u64* mom = (ls_u64*)moments_out_dev;
    if (elem_bytes == 1) return ls_run(e, (const uint8_t*)labels_dev, Z, H, W, capacity, mode, labels_out_dev, mom, stats_out_dev, out_n_labels, s);
    if (elem_bytes == 2 && is_signed) return ls_run(e, (const int16_t*)labels_dev, Z, H, W, capacity, mode, labels_out_dev, mom, stats_out_dev, out_n_labels, s);
    if (elem_bytes == 2) return ls_run(e, (const uint16_t*)labels_dev, Z, H, W, capacity, mode, labels_out_dev, mom, stats_out_dev, out_n_labels, s);
    if (is_signed) return ls_run(e, (const int32_t*)labels_dev, Z, H, W, capacity, mode, labels_out_dev, mom, stats_out_dev, out_n_labels, s);
    return ls_run(e, (const uint32_t*)labels_dev, Z, H, W, capacity, mode, labels_out_dev, mom, stats_out_dev, out_n_labels, s);
}
