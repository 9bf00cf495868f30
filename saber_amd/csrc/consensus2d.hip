// Consensus mask resolution on the device: overlap-averaged confidence, 4-connected 2-D components of the union, per-component table.
// Replaces the host arithmetic of saber.filters.masks._consensus_based_resolution (saber/filters/masks.py:64-121): the per-mask
// `confidence_map += seg * conf` / `overlap_count += seg` passes (:77-80), scipy.ndimage.label of the union (:88) and, per component,
// `labeled == lab`, np.mean, np.where and np.sum over the whole image (:92-105).  The image is read a fixed number of times whatever
// the number of masks' components is, and nothing of the size of the mask stack is allocated.
//
// Arithmetic model (bit for bit the reference's up to the per-component sum):
//   cm     float32, the confidences of the set masks added one after the other in list order (adding the 0 of an unset mask is exact,
//          so the chain over the set masks alone gives the reference's bits); adds only, nothing an fma could contract
//   count  int32 number of set masks
//   avg    (double)cm / (double)count, IEEE division (np.divide(float32, int32) is a float64 division), 0 where count = 0
//   score  the reference takes np.mean(avg[component]); here sum(avg) is accumulated per component in fp64 and the caller divides by
//          the area.  The sum's order differs from numpy's pairwise one (and, with atomics, between calls): both lie within the
//          any-order bound area * 2^-53 / (1 - area * 2^-53) * sum|avg| of the exact sum.
//
// Kernels (the union-find with min-index roots of ccl.h: a component's root IS its first pixel in raster order):
//   cs_accum    one wave per 256-pixel segment of a row: cm, count, avg; every foreground pixel starts as a child of the first pixel
//               of its x-run within the segment.  Two forms of the mask read, one body: a (n,H,W) uint8 stack, or rows of the mask
//               generator's bit-packed (n,H,W32) stack (saber_consensus_components_bits: a lane tests its bit of the word its half of
//               the 64-pixel chunk shares, an eighth of the bytes); the arithmetic above is the same statements in both
//   cs_merge    per pixel, the centre neighbour of the row above only (4-connectivity), and only at the first column a run shares
//               with the run above it; the left neighbour at a segment's first pixel
//   cs_flatten  parent <- root; a wave covers 64 consecutive pixels, so the ballot of "is a root" IS one 64-bit word of the root bitmap
//               (and adds its population count to the sum of its group of 1024 words: one integer atomic per word that holds a root)
//   cs_rank_groups / cs_rank_words   exclusive prefix sum of the words' population counts in two levels (one block over the group sums;
//               one block per group).  label(root r) = 1 + rankbase[r >> 6] + popc(bits below r): raster order of the first pixels,
//               scipy's numbering, without a sort.  counters[0] = K
//   cs_relabel  root -> label in place (the caller's int32 plane is the union-find array), and the identity rows of the table
//   cs_stats    one wave per 256-pixel segment of a row: consecutive set pixels of a row belong to one component, so a segmented wave
//               scan sums avg over each x-run in a fixed order and a run that crosses 64-pixel chunks is carried along: one table
//               update (area, box, fp64 sum) per run and segment, combined per block of 16 rows in LDS before it goes to global memory.  Rows past the caller's capacity are dropped on the device, so the host never has to know
//               K before the last launch.
//   cs_paint    saber_relabel_plane: plane[p] = lut[labels[p]], the classified slice's paint (components are disjoint, so painting the
//               area-sorted survivors one after the other is a table look-up)
// Host synchronisations per call: 1 (the end of the call, which brings K); saber_relabel_plane: none.
#include <algorithm>
#include <string>

#include "ccl.h"
#include "common.h"
#include "engine.h"

#define CS_GROUP_SHIFT 10        // bitmap words per group of the two-level rank (1024 words = 65536 pixels)

typedef unsigned long long cs_u64;

// One wave per segment of CS_SEG pixels of a row (a wave per row leaves a 1024-row image with one wave per SIMD, waiting on its own
// loads).  sel / conf are wave-uniform reads.  A lane owns CS_CPL pixels 64 apart, so a mask costs it CS_CPL independent byte loads and the
// loads of successive masks do not wait for each other either: only the fp32 adds of one pixel form a chain.  Runs start anew at a
// segment's first pixel; cs_merge joins them across the seam.
#define CS_CPL 4
#define CS_SEG (64 * CS_CPL)
// BITS: `masks` is a bit-packed stack (bit b of word w of a row = pixel 32w+b, W32 words per row, `stride` words per mask) instead of
// a uint8 one (`stride` = H W bytes per mask).  A segment starts at a multiple of 256 pixels and a chunk at a multiple of 64, so lanes
// 0..31 of a chunk share one word and lanes 32..63 the next; a pixel inside the row (in[i]) has its word inside the row.
template <bool BITS>
__global__ __launch_bounds__(256) void cs_accum_kernel(const void* __restrict__ masks, size_t stride, int W32, const int* __restrict__ sel,
                                                       const float* __restrict__ conf, int k, int W, int nseg, int64_t pieces, double* __restrict__ avg,
                                                       uint32_t* __restrict__ lab) {
    const int lane = threadIdx.x & 63;
    const int64_t piece = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (piece >= pieces) return;                               // wave-uniform
    const int64_t base = piece / nseg * W;
    uint32_t carry = CCL_NONE;                                 // start of the run that reaches the previous chunk's last pixel
    {
        const int xs = (int)(piece % nseg) * CS_SEG;
        float cm[CS_CPL];
        int cnt[CS_CPL];
        bool in[CS_CPL];
#pragma unroll
        for (int i = 0; i < CS_CPL; ++i) { cm[i] = 0.0f; cnt[i] = 0; in[i] = xs + 64 * i + lane < W; }
        if (BITS) {
            const uint32_t* p = (const uint32_t*)masks + piece / nseg * W32 + (xs >> 5) + (lane >> 5);
            const int bit = lane & 31;
#pragma unroll 2
            for (int j = 0; j < k; ++j) {
                const uint32_t* q = p + (size_t)sel[j] * stride;
                const float c = conf[j];
#pragma unroll
                for (int i = 0; i < CS_CPL; ++i)
                    if (in[i] && ((q[2 * i] >> bit) & 1u)) { cm[i] = __fadd_rn(cm[i], c); ++cnt[i]; }
            }
        } else {
            const uint8_t* p = (const uint8_t*)masks + base + xs + lane;
#pragma unroll 2
            for (int j = 0; j < k; ++j) {
                const uint8_t* q = p + (size_t)sel[j] * stride;
                const float c = conf[j];
#pragma unroll
                for (int i = 0; i < CS_CPL; ++i)
                    if (in[i] && q[64 * i]) { cm[i] = __fadd_rn(cm[i], c); ++cnt[i]; }
            }
        }
#pragma unroll
        for (int i = 0; i < CS_CPL; ++i) {
            const int x0 = xs + 64 * i;
            if (x0 >= W) break;                                // wave-uniform
            const int x = x0 + lane;
            const bool fg = cnt[i] > 0;
            const uint32_t start = ccl_run_start(fg, lane, (uint32_t)(base + x0), carry);
            if (fg) {
                lab[base + x] = start;
                avg[base + x] = __ddiv_rn((double)cm[i], (double)cnt[i]);
            } else if (x < W) {
                lab[base + x] = CCL_NONE;
                avg[base + x] = 0.0;
            }
        }
    }
}

__global__ __launch_bounds__(256) void cs_merge_kernel(uint32_t* lab, int W, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        if (lab[v] == CCL_NONE) continue;
        const int x = (int)(v % W);
        const bool left = x != 0 && lab[v - 1] != CCL_NONE;
        if (left && x % CS_SEG == 0) ccl_unite(lab, (uint32_t)v, (uint32_t)(v - 1));      // the seam between two segments of cs_accum
        if (v < W || lab[v - W] == CCL_NONE) continue;
        // the run of v and the run above it are joined at the first column they share: x = 0, or one of the two runs begins here
        if (left && lab[v - W - 1] != CCL_NONE) continue;
        ccl_unite(lab, (uint32_t)v, (uint32_t)(v - W));
    }
}

__global__ __launch_bounds__(256) void cs_flatten_kernel(uint32_t* lab, int64_t n, int64_t chunks, cs_u64* __restrict__ bitmap, uint32_t* groupsum) {
    const int lane = threadIdx.x & 63;
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < chunks; c += (int64_t)gridDim.x * 4) {   // wave-uniform
        const int64_t v = c * 64 + lane;
        uint32_t p = v < n ? lab[v] : CCL_NONE;
        bool root = false;
        if (p != CCL_NONE) {
            p = ccl_root(lab, p);
            lab[v] = p;
            root = p == (uint32_t)v;
        }
        const cs_u64 bits = __ballot(root);
        if (lane == 0) {
            bitmap[c] = bits;
            if (bits) atomicAdd(&groupsum[c >> CS_GROUP_SHIFT], (uint32_t)__popcll(bits));   // roots are few: one add per component, not per word
        }
    }
}

// one block of 1024 threads, in place: groupsum[g] (roots in the CS_GROUP words of group g) -> roots in the groups below g; counters[0] = K
__global__ __launch_bounds__(1024) void cs_rank_groups_kernel(uint32_t* __restrict__ groupsum, int64_t ng, uint32_t* __restrict__ counters) {
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (ng + 1023) / 1024;
    const int64_t g0 = min((int64_t)t * per, ng), g1 = min(g0 + per, ng);
    uint32_t s = 0;
    for (int64_t g = g0; g < g1; ++g) s += groupsum[g];
    part[t] = s;
    block_scan_inclusive<1024>(part, t);
    uint32_t run = part[t] - s;
    for (int64_t g = g0; g < g1; ++g) { const uint32_t c = groupsum[g]; groupsum[g] = run; run += c; }
    if (t == 1023) counters[0] = part[1023];
}

// one block per group of CS_GROUP bitmap words, 4 consecutive words per thread: rankbase[w] = roots in the words below w
__global__ __launch_bounds__(256) void cs_rank_words_kernel(const cs_u64* __restrict__ bitmap, int64_t nw, const uint32_t* __restrict__ groupbase,
                                                            uint32_t* __restrict__ rankbase) {
    __shared__ uint32_t part[256];
    const int t = threadIdx.x;
    const int64_t w0 = ((int64_t)blockIdx.x << CS_GROUP_SHIFT) + 4 * t;
    uint32_t c[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { c[i] = w0 + i < nw ? (uint32_t)__popcll(bitmap[w0 + i]) : 0u; s += c[i]; }
    part[t] = s;
    block_scan_inclusive<256>(part, t);
    uint32_t run = groupbase[blockIdx.x] + part[t] - s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (w0 + i < nw) rankbase[w0 + i] = run;
        run += c[i];
    }
}

__global__ __launch_bounds__(256) void cs_relabel_kernel(uint32_t* lab, int64_t n, const cs_u64* __restrict__ bitmap, const uint32_t* __restrict__ rankbase,
                                                         const uint32_t* __restrict__ counters, int capacity, saber_consensus_row* __restrict__ table) {
    const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t v = t0; v < n; v += stride) {
        const uint32_t r = lab[v];                             // a pixel reads and writes its own entry only
        lab[v] = r == CCL_NONE ? 0u : 1u + rankbase[r >> 6] + (uint32_t)__popcll(bitmap[r >> 6] & ((1ull << (r & 63)) - 1ull));
    }
    const int64_t rows = min((int64_t)counters[0], (int64_t)capacity);
    for (int64_t i = t0; i < rows; i += stride) {
        saber_consensus_row id;
        id.area = 0; id.x_min = 0x7fffffff; id.y_min = 0x7fffffff; id.x_max = -1; id.y_max = -1; id.reserved = 0; id.avg_sum = 0.0;
        table[i] = id;
    }
}

__device__ __forceinline__ void cs_flush(saber_consensus_row* table, int capacity, int label, int area, int x_min, int x_max, int y, double sum) {
    if ((uint32_t)(label - 1) >= (uint32_t)capacity) return;
    saber_consensus_row* r = table + (label - 1);
    atomicAdd(&r->area, area);
    atomicMin(&r->x_min, x_min);
    atomicMax(&r->x_max, x_max);
    atomicMin(&r->y_min, y);
    atomicMax(&r->y_max, y);
    atomicAdd(&r->avg_sum, sum);
}

// A block of 16 waves covers 16 rows of one 256-pixel segment; wave = row.  Updates of a component meet in the block's LDS table first
// (direct-mapped by label; a label that finds its slot taken by another goes to global memory directly), so what reaches the global
// table is one update per block and component: the global atomics of one component all hit the same 32 bytes and queue up there.
#define CS_STAT_ROWS 16
#define CS_SLOTS 32
__global__ __launch_bounds__(64 * CS_STAT_ROWS) void cs_stats_kernel(const int32_t* __restrict__ labels, const double* __restrict__ avg, int W, int H,
                                                                     int nseg, int capacity, saber_consensus_row* table) {
    __shared__ int t_tag[CS_SLOTS], t_area[CS_SLOTS], t_x0[CS_SLOTS], t_y0[CS_SLOTS], t_x1[CS_SLOTS], t_y1[CS_SLOTS];
    __shared__ double t_sum[CS_SLOTS];
    if (threadIdx.x < CS_SLOTS) {
        const int i = threadIdx.x;
        t_tag[i] = 0; t_area[i] = 0; t_x0[i] = 0x7fffffff; t_y0[i] = 0x7fffffff; t_x1[i] = -1; t_y1[i] = -1; t_sum[i] = 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int row = (int)(blockIdx.x / nseg) * CS_STAT_ROWS + (threadIdx.x >> 6);
    const int xs = (int)(blockIdx.x % nseg) * CS_SEG, xe = min(W, xs + CS_SEG);
    auto flush = [&](int label, int area, int x_min, int x_max, double sum) {
        if ((uint32_t)(label - 1) >= (uint32_t)capacity) return;
        const int slot = label & (CS_SLOTS - 1);
        const int old = atomicCAS(&t_tag[slot], 0, label);
        if (old == 0 || old == label) {
            atomicAdd(&t_area[slot], area);
            atomicMin(&t_x0[slot], x_min);
            atomicMax(&t_x1[slot], x_max);
            atomicMin(&t_y0[slot], row);
            atomicMax(&t_y1[slot], row);
            atomicAdd(&t_sum[slot], sum);
        } else cs_flush(table, capacity, label, area, x_min, x_max, row, sum);
    };
    if (row < H) {                                             // wave-uniform
        const int64_t base = (int64_t)row * W;
        int ls[CS_CPL];
        double as[CS_CPL];
#pragma unroll
        for (int i = 0; i < CS_CPL; ++i) {                     // every load of the segment is issued before the first is used
            const int x = xs + 64 * i + lane;
            ls[i] = x < xe ? labels[base + x] : 0;
        }
#pragma unroll
        for (int i = 0; i < CS_CPL; ++i) as[i] = ls[i] > 0 ? avg[base + xs + 64 * i + lane] : 0.0;
        // the run that reached the previous chunk's last pixel and may go on in this one (wave-uniform)
        int open = 0, c_label = 0, c_area = 0, c_xmin = 0;
        double c_sum = 0.0;
#pragma unroll
        for (int i = 0; i < CS_CPL; ++i) {
            const int x0 = xs + 64 * i;
            if (x0 >= xe) break;                               // wave-uniform
            const int x = x0 + lane;
            const int l = ls[i];
            const bool fg = l > 0;
            const cs_u64 mask = __ballot(fg);
            if (!mask && !open) continue;                      // wave-uniform: an empty chunk with nothing carried into it
            double s = as[i];
            const cs_u64 below_bg = ~mask & ((1ull << lane) - 1ull);
            const int h = below_bg ? 64 - __clzll((long long)below_bg) : 0;      // first lane of this lane's run
            // segmented inclusive scan: lane L ends with the sum over lanes h..L of its run, in an order fixed by the run's position
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double t = __shfl_up(s, o, 64);
                if (lane - o >= h) s += t;
            }
            const bool tail = fg && (lane == 63 || !((mask >> (lane + 1)) & 1ull));
            int area = lane - h + 1, x_min = x0 + h;
            if (open) {
                if (mask & 1ull) {
                    if (fg && h == 0) { s = c_sum + s; area += c_area; x_min = c_xmin; }
                } else if (lane == 0) flush(c_label, c_area, c_xmin, x0 - 1, c_sum);
            }
            const bool defer = tail && lane == 63 && x + 1 < xe;   // may continue in the wave's next chunk
            if (tail && !defer) flush(l, area, x_min, x, s);
            open = __shfl((int)defer, 63, 64);
            if (open) {
                c_sum = __shfl(s, 63, 64);
                c_area = __shfl(area, 63, 64);
                c_xmin = __shfl(x_min, 63, 64);
                c_label = __shfl(l, 63, 64);
            }
        }                                                      // the segment's last chunk never defers: nothing is open here
    }
    __syncthreads();
    if (threadIdx.x < CS_SLOTS && t_tag[threadIdx.x] != 0) {
        const int i = threadIdx.x;
        saber_consensus_row* r = table + (t_tag[i] - 1);       // a tag passed the capacity test when it was set
        atomicAdd(&r->area, t_area[i]);
        atomicMin(&r->x_min, t_x0[i]);
        atomicMax(&r->x_max, t_x1[i]);
        atomicMin(&r->y_min, t_y0[i]);
        atomicMax(&r->y_max, t_y1[i]);
        atomicAdd(&r->avg_sum, t_sum[i]);
    }
}

// plane[p] = lut[labels[p]] (lut[0] = 0: background); a label past the table paints nothing
__global__ __launch_bounds__(256) void cs_paint_kernel(const int32_t* __restrict__ labels, int64_t n, const uint16_t* __restrict__ lut, int L,
                                                       uint16_t* __restrict__ plane) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const int32_t l = labels[v];
        plane[v] = (uint32_t)l < (uint32_t)L ? lut[l] : (uint16_t)0;
    }
}

namespace {
inline size_t cs_align(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

// both entries: `bits` says which of the two stacks masks_dev is; `who` names the entry in the error strings
static int cs_components(saber_engine* e, const std::string& who, const void* masks_dev, bool bits, int n, int H, int W, const int* select_host,
                         const float* conf_host, int k, int capacity, int32_t* labels_out_dev, saber_consensus_row* table_out_dev,
                         int* out_n_components, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (out_n_components) *out_n_components = 0;
    if (!masks_dev || !select_host || !conf_host || !labels_out_dev || capacity < 0 || (capacity > 0 && !table_out_dev))
        return eng_fail(e, SABER_ERR_INVALID, who + ": bad argument");
    if (n < 1 || H < 1 || W < 1) return eng_fail(e, SABER_ERR_INVALID, who + ": n, H and W must be at least 1");
    const int64_t npx = (int64_t)H * W;
    if (npx >= (int64_t)0x7fffffff) return eng_fail(e, SABER_ERR_INVALID, who + ": images of 2^31 pixels or more are not supported");
    if (k < 1 || k > n) return eng_fail(e, SABER_ERR_INVALID, who + ": the selection must hold 1..n masks, got " + std::to_string(k));
    for (int j = 0; j < k; ++j)
        if (select_host[j] < 0 || select_host[j] >= n)
            return eng_fail(e, SABER_ERR_INVALID, who + ": selected index " + std::to_string(select_host[j]) + " is outside the stack of " + std::to_string(n));
    hipStream_t s = (hipStream_t)stream;
    ENG_DEVICE(e);
    const int64_t nw = (npx + 63) / 64;
    const int64_t ng = (nw + (1 << CS_GROUP_SHIFT) - 1) >> CS_GROUP_SHIFT;
    const size_t off_bitmap = cs_align((size_t)npx * 8), off_rank = off_bitmap + cs_align((size_t)nw * 8), off_group = off_rank + cs_align((size_t)nw * 4);
    const size_t off_cnt = off_group + cs_align((size_t)ng * 4);
    const size_t off_sel = off_cnt + 256, off_conf = off_sel + cs_align((size_t)k * 4), total = off_conf + cs_align((size_t)k * 4);
    if (e->consensus_ws_bytes < total) {
        if (e->consensus_ws) {
            ENG_HIP(e, hipStreamSynchronize(s));               // a larger image than any before: the old workspace may still be in use
            eng_free(e, e->consensus_ws);
            e->consensus_ws = nullptr;
            e->consensus_ws_bytes = 0;
        }
        void* p = nullptr;
        const int st = eng_alloc_bytes(e, &p, total);
        if (st != SABER_OK) return st;
        e->consensus_ws = p;
        e->consensus_ws_bytes = total;
    }
    char* ws = (char*)e->consensus_ws;
    double* avg = (double*)ws;
    cs_u64* bitmap = (cs_u64*)(ws + off_bitmap);
    uint32_t* rankbase = (uint32_t*)(ws + off_rank);
    uint32_t* groups = (uint32_t*)(ws + off_group);
    uint32_t* counters = (uint32_t*)(ws + off_cnt);
    int* sel = (int*)(ws + off_sel);
    float* conf = (float*)(ws + off_conf);
    uint32_t* lab = (uint32_t*)labels_out_dev;
    ENG_HIP(e, hipMemcpyAsync(sel, select_host, (size_t)k * 4, hipMemcpyHostToDevice, s));
    ENG_HIP(e, hipMemcpyAsync(conf, conf_host, (size_t)k * 4, hipMemcpyHostToDevice, s));
    ENG_HIP(e, hipMemsetAsync(groups, 0, (size_t)ng * 4, s));
    const int nseg = (W + CS_SEG - 1) / CS_SEG;
    const int64_t pieces = (int64_t)H * nseg;
    const unsigned piece_blocks = (unsigned)((pieces + 3) / 4), px_blocks = eng_blocks(npx);
    const int W32 = (W + 31) / 32;
    if (bits)
        hipLaunchKernelGGL(cs_accum_kernel<true>, dim3(piece_blocks), dim3(256), 0, s, masks_dev, (size_t)H * W32, W32, (const int*)sel, (const float*)conf, k, W, nseg,
                           pieces, avg, lab);
    else
        hipLaunchKernelGGL(cs_accum_kernel<false>, dim3(piece_blocks), dim3(256), 0, s, masks_dev, (size_t)npx, W32, (const int*)sel, (const float*)conf, k, W, nseg,
                           pieces, avg, lab);
    if (H > 1 || nseg > 1) hipLaunchKernelGGL(cs_merge_kernel, dim3(px_blocks), dim3(256), 0, s, lab, W, npx);
    hipLaunchKernelGGL(cs_flatten_kernel, dim3(eng_blocks(nw * 64)), dim3(256), 0, s, lab, npx, nw, bitmap, groups);
    hipLaunchKernelGGL(cs_rank_groups_kernel, dim3(1), dim3(1024), 0, s, groups, ng, counters);
    hipLaunchKernelGGL(cs_rank_words_kernel, dim3((unsigned)ng), dim3(256), 0, s, (const cs_u64*)bitmap, nw, (const uint32_t*)groups, rankbase);
    hipLaunchKernelGGL(cs_relabel_kernel, dim3(px_blocks), dim3(256), 0, s, lab, npx, (const cs_u64*)bitmap, (const uint32_t*)rankbase,
                       (const uint32_t*)counters, capacity, table_out_dev);
    if (capacity > 0)
        hipLaunchKernelGGL(cs_stats_kernel, dim3((unsigned)(((int64_t)H + CS_STAT_ROWS - 1) / CS_STAT_ROWS * nseg)), dim3(64 * CS_STAT_ROWS), 0, s,
                           (const int32_t*)labels_out_dev, (const double*)avg, W, H, nseg, capacity, table_out_dev);
    ENG_HIP(e, hipGetLastError());
    uint32_t K = 0;
    ENG_HIP(e, hipMemcpyAsync(&K, counters, 4, hipMemcpyDeviceToHost, s));
    ENG_HIP(e, hipStreamSynchronize(s));                        // the call's one synchronisation
    if (out_n_components) *out_n_components = (int)K;
    if ((int64_t)K > capacity)
        return eng_fail(e, SABER_ERR_CAPACITY, who + ": the union has " + std::to_string(K) + " components, the table has room for " +
                                                   std::to_string(capacity));
    return SABER_OK;
}

extern "C" int saber_consensus_components(saber_engine* e, const uint8_t* masks_dev, int n, int H, int W, const int* select_host,
                                          const float* conf_host, int k, int capacity, int32_t* labels_out_dev, saber_consensus_row* table_out_dev,
                                          int* out_n_components, void* stream) {
    return cs_components(e, "consensus_components", masks_dev, false, n, H, W, select_host, conf_host, k, capacity, labels_out_dev, table_out_dev,
                         out_n_components, stream);
}

extern "C" int saber_consensus_components_bits(saber_engine* e, const uint32_t* bits_dev, int n_rows, int H, int W, const int* select_host,
                                               const float* conf_host, int k, int capacity, int32_t* labels_out_dev, saber_consensus_row* table_out_dev,
                                               int* out_n_components, void* stream) {
    return cs_components(e, "consensus_components_bits", bits_dev, true, n_rows, H, W, select_host, conf_host, k, capacity, labels_out_dev, table_out_dev,
                         out_n_components, stream);
}

extern "C" int saber_relabel_plane(saber_engine* e, const int32_t* labels_dev, int H, int W, const uint16_t* lut_dev, int lut_len, uint16_t* plane_dev,
                                   void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!labels_dev || !lut_dev || !plane_dev || H < 1 || W < 1 || lut_len < 1) return eng_fail(e, SABER_ERR_INVALID, "relabel_plane: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ENG_DEVICE(e);
    const int64_t npx = (int64_t)H * W;
    hipLaunchKernelGGL(cs_paint_kernel, dim3(eng_blocks(npx)), dim3(256), 0, s, labels_dev, npx, lut_dev, lut_len, plane_dev);
    ENG_HIP(e, hipGetLastError());
    return SABER_OK;
}
