// 3-D connected components of the stitched label volume on the device.
// Replaces saber.segmenters.utils.separate_masks (saber/segmenters/utils.py:88-131; called at the end of the slice loop,
// propagation.py:189, and of the tomogram path, tomo.py:248): foreground = label != 0 (touching objects stay merged),
// 26-connectivity, components below min_mask_area * 10 voxels removed, survivors renumbered 1..K in the order scipy.ndimage.label
// meets them (C-order scan = ascending index of a component's first voxel), uint32 output.  Integer work: bit-exact.
//
// The labelling is the union-find with min-index roots of ccl.h (a component's root IS its first voxel in scan order):
//   1-4. ccl_init, cc_merge, ccl_flatten, ccl_count   the merge looks, per voxel, at the 4 rows that precede it in scan order
//                   ((z,y-1), (z-1,y-1), (z-1,y), (z-1,y+1)); per row only the centre neighbour if it is foreground (its x-neighbours
//                   hang on the same run), else the two diagonals.  The voxel counts accumulate in the OUTPUT buffer at the root's index
//   5. cc_roots     roots with >= min_vol voxels are appended to a list, the others get id 0; the host sorts the (short) list
//   6. cc_assign / cc_relabel   id = rank in the sorted list + 1; out[v] = id[root(v)] in place (a root's own entry already holds its id)
#include <algorithm>
#include <vector>

#include "ccl.h"
#include "engine.h"

__global__ __launch_bounds__(256) void cc_merge_kernel(const uint16_t* __restrict__ planes, uint32_t* __restrict__ lab, int Z, int H, int W) {
    const int64_t n = (int64_t)Z * H * W;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        if (planes[v] == 0) continue;
        const int x = (int)(v % W);
        const int64_t r = v / W;
        const int y = (int)(r % H), z = (int)(r / H);
        // rows that precede (z, y) in scan order and touch it
        const int dz[4] = {0, -1, -1, -1}, dy[4] = {-1, -1, 0, 1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int zz = z + dz[k], yy = y + dy[k];
            if (zz < 0 || yy < 0 || yy >= H) continue;
            const int64_t rb = ((int64_t)zz * H + yy) * W;
            if (planes[rb + x] != 0) { ccl_unite(lab, (uint32_t)v, (uint32_t)(rb + x)); continue; }
            if (x > 0 && planes[rb + x - 1] != 0) ccl_unite(lab, (uint32_t)v, (uint32_t)(rb + x - 1));
            if (x + 1 < W && planes[rb + x + 1] != 0) ccl_unite(lab, (uint32_t)v, (uint32_t)(rb + x + 1));
        }
    }
}

__global__ __launch_bounds__(256) void cc_roots_kernel(const uint32_t* __restrict__ lab, uint32_t* __restrict__ sizes, int64_t n, uint32_t min_vol,
                                                       uint32_t* __restrict__ list, uint32_t cap, uint32_t* __restrict__ counter) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        if (lab[v] != (uint32_t)v) continue;                   // roots only
        if (sizes[v] >= min_vol) {
            const uint32_t i = atomicAdd(counter, 1u);
            if (i < cap) list[i] = (uint32_t)v;
        } else sizes[v] = 0u;                                   // removed component: id 0
    }
}

__global__ __launch_bounds__(256) void cc_assign_kernel(const uint32_t* __restrict__ sorted_roots, uint32_t k, uint32_t* __restrict__ ids) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < k) ids[sorted_roots[i]] = i + 1u;
}

__global__ __launch_bounds__(256) void cc_relabel_kernel(const uint32_t* __restrict__ lab, uint32_t* __restrict__ out, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const uint32_t r = lab[v];
        if (r == CCL_NONE) out[v] = 0u;
        else if (r != (uint32_t)v) out[v] = out[r];            // a root's own entry already holds its id and is only ever re-written with it
    }
}

// init / merge / flatten / count of one (Z,H,W) block of planes: lab[v] = the block's root of v (CCL_NONE for background), sizes[root] =
// its voxel count.  Only enqueues; the caller checks hipGetLastError.
static void cc_label(const uint16_t* planes_dev, uint32_t* lab, uint32_t* sizes, int Z, int H, int W, hipStream_t s) {
    const int64_t n = (int64_t)Z * H * W, rows = (int64_t)Z * H;
    const unsigned vox_blocks = eng_blocks(n, 1 << 20);
    ccl_init(planes_dev, lab, nullptr, nullptr, W, rows, s);
    hipLaunchKernelGGL(cc_merge_kernel, dim3(vox_blocks), dim3(256), 0, s, planes_dev, lab, Z, H, W);
    ccl_flatten(lab, n, vox_blocks, s);
    ccl_count(lab, sizes, W, rows, s);
}

// utils.py:113
static uint32_t cc_min_vol(int min_mask_area) { return min_mask_area > 0 ? (uint32_t)std::min<int64_t>((int64_t)min_mask_area * 10, 0x7fffffff) : 0u; }
// length of the root list: a kept component has >= max(min_vol, 1) voxels; isolated voxels of a 26-connected labelling are >= 2 apart in every axis
static int64_t cc_root_cap(int64_t n, int Z, int H, int W, uint32_t min_vol) {
    return min_vol > 1 ? n / min_vol + 1 : (int64_t)((Z + 1) / 2) * ((H + 1) / 2) * ((W + 1) / 2) + 1;
}

extern "C" int saber_separate_masks(saber_engine* e, const uint16_t* planes_dev, int Z, int H, int W, int min_mask_area, uint32_t* out_dev,
                                    int* out_n_labels, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!planes_dev || !out_dev || Z <= 0 || H <= 0 || W <= 0) return eng_fail(e, SABER_ERR_INVALID, "separate_masks: bad argument");
    const int64_t n = (int64_t)Z * H * W;
    if (n >= (int64_t)0x7fffffff) return eng_fail(e, SABER_ERR_INVALID, "separate_masks: volumes of 2^31 voxels or more are not supported");
    if (out_n_labels) *out_n_labels = 0;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *lab = nullptr, *list = nullptr, *counter = nullptr;
    auto cleanup = [&]() { (void)hipFree(lab); (void)hipFree(list); (void)hipFree(counter); };
    ENG_DEVICE(e);
    const uint32_t min_vol = cc_min_vol(min_mask_area);
    const uint32_t cap = (uint32_t)cc_root_cap(n, Z, H, W, min_vol);
    ENG_HIP_CLEANUP(e, hipMalloc(&lab, (size_t)n * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&list, (size_t)cap * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&counter, 4));
    ENG_HIP_CLEANUP(e, hipMemsetAsync(counter, 0, 4, s));
    ENG_HIP_CLEANUP(e, hipMemsetAsync(out_dev, 0, (size_t)n * 4, s));
    const unsigned vox_blocks = eng_blocks(n, 1 << 20);
    cc_label(planes_dev, lab, out_dev, Z, H, W, s);
    hipLaunchKernelGGL(cc_roots_kernel, dim3(vox_blocks), dim3(256), 0, s, (const uint32_t*)lab, out_dev, n, std::max(min_vol, 1u), list, cap, counter);
    uint32_t k = 0;
    ENG_HIP_CLEANUP(e, hipMemcpyAsync(&k, counter, 4, hipMemcpyDeviceToHost, s));
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
    if (k > cap) { cleanup(); return eng_fail(e, SABER_ERR_CAPACITY, "separate_masks: internal root list overflow"); }
    if (k > 0) {
        std::vector<uint32_t> roots(k);
        ENG_HIP_CLEANUP(e, hipMemcpyAsync(roots.data(), list, (size_t)k * 4, hipMemcpyDeviceToHost, s));
        ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
        std::sort(roots.begin(), roots.end());                 // ascending first-voxel index = scipy's label order
        ENG_HIP_CLEANUP(e, hipMemcpyAsync(list, roots.data(), (size_t)k * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(cc_assign_kernel, dim3((k + 255) / 256), dim3(256), 0, s, (const uint32_t*)list, k, out_dev);
        ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));                    // `roots` must outlive the upload
    }
    hipLaunchKernelGGL(cc_relabel_kernel, dim3(vox_blocks), dim3(256), 0, s, (const uint32_t*)lab, out_dev, n);
    ENG_HIP_CLEANUP(e, hipGetLastError());
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
    cleanup();
    if (out_n_labels) *out_n_labels = (int)k;
    return SABER_OK;
}

// ---- the sharded stitch: the same labelling on one z-chunk of the volume, and what joins the chunks across a seam --------------------
// A chunk is labelled on its own (saber_cc_chunk_label).  Its roots are chunk-local first voxels; z-chunks are contiguous in scan order, so
// root + z0*H*W is a global voxel index and a component that spans chunks has the minimum of its pieces' roots as its global first voxel.
// What touches across the seam between two chunks comes from cc_seam_pairs_kernel on the two facing root planes; the host joins the pairs
// (saber_amd/segmenters/stitch.py) and hands every chunk the ids of its roots (saber_cc_chunk_finish).

// ids[roots[i]] = values[i], or 0 without values.  Roots past n are skipped (the host has rejected them already).
__global__ __launch_bounds__(256) void cc_assign_list_kernel(const uint32_t* __restrict__ roots, const uint32_t* __restrict__ values, uint32_t k,
                                                             uint32_t* __restrict__ ids, int64_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const uint32_t r = roots[i];
    if ((int64_t)r < n) ids[r] = values ? values[i] : 0u;
}

// Pairs (root in a, root in b) of the foreground pixels of plane a (a chunk's last plane) and plane b (the next chunk's first plane) that
// touch across the seam: |dy| <= 1, |dx| <= 1.  Per row offset dy the rule is cc_merge_kernel's: the centre neighbour if it is foreground
// (its x-neighbours hang on the same run), else the two diagonals.  A pair is not emitted when the pixel's left neighbour emits the same
// pair for the same dy (along an x-run of a over an x-run of b every pixel would repeat it).  The emitted list may still hold repeats; the
// host removes them.  a_off / b_off are added to the roots (chunk-local index -> global index).
// One thread per pixel, whole waves (no early exit in front of the ballots).  A lane has up to 6 pairs (3 rows x 2); the wave sums the
// ballots of the 6 slots and takes its range with ONE counter add, lane 0's.  Pairs past `cap` are counted, not written: the host sees
// *counter > cap and asks again with room for all.
struct cc_row_emit { uint32_t r[2]; };
__device__ __forceinline__ cc_row_emit cc_seam_row(uint32_t ra, const uint32_t* __restrict__ brow, int x, int W) {
    cc_row_emit o = {{CCL_NONE, CCL_NONE}};
    if (ra == CCL_NONE) return o;
    const uint32_t c = brow[x];
    if (c != CCL_NONE) { o.r[0] = c; return o; }
    if (x > 0) o.r[0] = brow[x - 1];
    if (x + 1 < W) o.r[1] = brow[x + 1];
    return o;
}
__global__ __launch_bounds__(256) void cc_seam_pairs_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, int H, int W, uint32_t a_off,
                                                            uint32_t b_off, uint32_t* __restrict__ pairs, uint32_t cap, uint32_t* __restrict__ counter) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = p < (int64_t)H * W;
    const int y = in ? (int)(p / W) : 0, x = in ? (int)(p % W) : 0;
    const uint32_t ra = in ? a[p] : CCL_NONE;
    const uint32_t rl = in && x > 0 ? a[p - 1] : CCL_NONE;         // the left neighbour's root
    uint32_t em[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int yy = y + k - 1;
        em[2 * k] = em[2 * k + 1] = CCL_NONE;
        if (ra == CCL_NONE || yy < 0 || yy >= H) continue;
        const uint32_t* brow = b + (int64_t)yy * W;
        const cc_row_emit me = cc_seam_row(ra, brow, x, W);
        cc_row_emit left = {{CCL_NONE, CCL_NONE}};
        if (rl == ra) left = cc_seam_row(rl, brow, x - 1, W);      // only a left neighbour with my root can emit my pairs
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (me.r[j] != CCL_NONE && me.r[j] != left.r[0] && me.r[j] != left.r[1]) em[2 * k + j] = me.r[j];
    }
    uint32_t total = 0, mine[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const unsigned long long m = __ballot(em[j] != CCL_NONE);
        mine[j] = total + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        total += (uint32_t)__popcll(m);
    }
    if (total == 0u) return;                                       // wave-uniform
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(counter, total);
    base = __shfl(base, 0, 64);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const uint32_t i = base + mine[j];
        if (em[j] != CCL_NONE && i < cap) {
            pairs[2 * (size_t)i] = ra + a_off;
            pairs[2 * (size_t)i + 1] = em[j] + b_off;
        }
    }
}

static int cc_chunk_dims(saber_engine* e, const char* who, int Z, int H, int W, int64_t* n) {
    if (Z <= 0 || H <= 0 || W <= 0) return eng_fail(e, SABER_ERR_INVALID, std::string(who) + ": bad argument");
    *n = (int64_t)Z * H * W;
    if (*n >= (int64_t)0x7fffffff) return eng_fail(e, SABER_ERR_INVALID, std::string(who) + ": chunks of 2^31 voxels or more are not supported");
    return SABER_OK;
}
// every entry of a host root list must name a voxel of the chunk
static bool cc_roots_in_range(const uint32_t* roots, int k, int64_t n) {
    for (int i = 0; i < k; ++i)
        if ((int64_t)roots[i] >= n) return false;
    return true;
}

extern "C" int saber_cc_chunk_label(saber_engine* e, const uint16_t* planes_dev, int Z, int H, int W, uint32_t* lab_dev, uint32_t* sizes_dev,
                                    void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!planes_dev || !lab_dev || !sizes_dev) return eng_fail(e, SABER_ERR_INVALID, "cc_chunk_label: bad argument");
    int64_t n = 0;
    if (int st = cc_chunk_dims(e, "cc_chunk_label", Z, H, W, &n)) return st;
    hipStream_t s = (hipStream_t)stream;
    ENG_DEVICE(e);
    ENG_HIP(e, hipMemsetAsync(sizes_dev, 0, (size_t)n * 4, s));
    cc_label(planes_dev, lab_dev, sizes_dev, Z, H, W, s);
    ENG_HIP(e, hipGetLastError());
    return SABER_OK;
}

extern "C" int saber_cc_seam_pairs(saber_engine* e, const uint32_t* a_roots_dev, const uint32_t* b_roots_dev, int H, int W, uint32_t a_offset,
                                   uint32_t b_offset, uint32_t* pairs_dev, int capacity, int* out_count, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!a_roots_dev || !b_roots_dev || !out_count || H <= 0 || W <= 0 || capacity < 0 || (capacity > 0 && !pairs_dev))
        return eng_fail(e, SABER_ERR_INVALID, "cc_seam_pairs: bad argument");
    if ((int64_t)H * W > (int64_t)0x7fffffff / 6) return eng_fail(e, SABER_ERR_INVALID, "cc_seam_pairs: plane too large (6 pairs per pixel must fit an int)");
    *out_count = 0;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* counter = nullptr;
    auto cleanup = [&]() { (void)hipFree(counter); };
    ENG_DEVICE(e);
    ENG_HIP_CLEANUP(e, hipMalloc(&counter, 4));
    ENG_HIP_CLEANUP(e, hipMemsetAsync(counter, 0, 4, s));
    hipLaunchKernelGGL(cc_seam_pairs_kernel, dim3((unsigned)(((int64_t)H * W + 255) / 256)), dim3(256), 0, s, a_roots_dev, b_roots_dev, H, W, a_offset,
                       b_offset, pairs_dev, (uint32_t)capacity, counter);
    ENG_HIP_CLEANUP(e, hipGetLastError());
    uint32_t k = 0;
    ENG_HIP_CLEANUP(e, hipMemcpyAsync(&k, counter, 4, hipMemcpyDeviceToHost, s));
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
    cleanup();
    *out_count = (int)k;
    if (k > (uint32_t)capacity)
        return eng_fail(e, SABER_ERR_CAPACITY, "cc_seam_pairs: " + std::to_string(k) + " pairs, the buffer holds " + std::to_string(capacity));
    return SABER_OK;
}

extern "C" int saber_cc_chunk_roots(saber_engine* e, const uint32_t* lab_dev, uint32_t* sizes_dev, int Z, int H, int W, uint32_t min_voxels,
                                    const uint32_t* exclude_host, int n_exclude, uint32_t* roots_out_host, int capacity, int* out_count, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!lab_dev || !sizes_dev || !out_count || n_exclude < 0 || (n_exclude > 0 && !exclude_host) || capacity < 0 || (capacity > 0 && !roots_out_host))
        return eng_fail(e, SABER_ERR_INVALID, "cc_chunk_roots: bad argument");
    int64_t n = 0;
    if (int st = cc_chunk_dims(e, "cc_chunk_roots", Z, H, W, &n)) return st;
    if (!cc_roots_in_range(exclude_host, n_exclude, n)) return eng_fail(e, SABER_ERR_INVALID, "cc_chunk_roots: an excluded root lies outside the chunk");
    *out_count = 0;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t min_vol = std::max(min_voxels, 1u);
    const uint32_t cap = (uint32_t)cc_root_cap(n, Z, H, W, min_vol);
    uint32_t *list = nullptr, *counter = nullptr, *excl = nullptr;
    auto cleanup = [&]() { (void)hipFree(list); (void)hipFree(counter); (void)hipFree(excl); };
    ENG_DEVICE(e);
    ENG_HIP_CLEANUP(e, hipMalloc(&list, (size_t)cap * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&counter, 4));
    ENG_HIP_CLEANUP(e, hipMemsetAsync(counter, 0, 4, s));
    if (n_exclude > 0) {
        // an excluded root's size is cleared: cc_roots_kernel then passes it by as it does a removed component (id 0 until assigned)
        ENG_HIP_CLEANUP(e, hipMalloc(&excl, (size_t)n_exclude * 4));
        ENG_HIP_CLEANUP(e, hipMemcpyAsync(excl, exclude_host, (size_t)n_exclude * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(cc_assign_list_kernel, dim3(((unsigned)n_exclude + 255) / 256), dim3(256), 0, s, (const uint32_t*)excl, (const uint32_t*)nullptr,
                           (uint32_t)n_exclude, sizes_dev, n);
    }
    hipLaunchKernelGGL(cc_roots_kernel, dim3(eng_blocks(n, 1 << 20)), dim3(256), 0, s, lab_dev, sizes_dev, n, min_vol, list, cap, counter);
    ENG_HIP_CLEANUP(e, hipGetLastError());
    uint32_t k = 0;
    ENG_HIP_CLEANUP(e, hipMemcpyAsync(&k, counter, 4, hipMemcpyDeviceToHost, s));
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
    if (k > cap) { cleanup(); return eng_fail(e, SABER_ERR_CAPACITY, "cc_chunk_roots: internal root list overflow"); }
    *out_count = (int)k;
    if (k > (uint32_t)capacity) {
        cleanup();
        return eng_fail(e, SABER_ERR_CAPACITY, "cc_chunk_roots: " + std::to_string(k) + " roots, the buffer holds " + std::to_string(capacity));
    }
    if (k > 0) {
        ENG_HIP_CLEANUP(e, hipMemcpyAsync(roots_out_host, list, (size_t)k * 4, hipMemcpyDeviceToHost, s));
        ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
        std::sort(roots_out_host, roots_out_host + k);
    }
    cleanup();
    return SABER_OK;
}

extern "C" int saber_cc_chunk_finish(saber_engine* e, const uint32_t* lab_dev, uint32_t* sizes_dev, int Z, int H, int W, const uint32_t* roots_host,
                                     const uint32_t* ids_host, int k, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!lab_dev || !sizes_dev || k < 0 || (k > 0 && (!roots_host || !ids_host))) return eng_fail(e, SABER_ERR_INVALID, "cc_chunk_finish: bad argument");
    int64_t n = 0;
    if (int st = cc_chunk_dims(e, "cc_chunk_finish", Z, H, W, &n)) return st;
    if (!cc_roots_in_range(roots_host, k, n)) return eng_fail(e, SABER_ERR_INVALID, "cc_chunk_finish: a root lies outside the chunk");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* up = nullptr;
    auto cleanup = [&]() { (void)hipFree(up); };
    ENG_DEVICE(e);
    if (k > 0) {
        ENG_HIP_CLEANUP(e, hipMalloc(&up, (size_t)k * 8));
        ENG_HIP_CLEANUP(e, hipMemcpyAsync(up, roots_host, (size_t)k * 4, hipMemcpyHostToDevice, s));
        ENG_HIP_CLEANUP(e, hipMemcpyAsync(up + k, ids_host, (size_t)k * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(cc_assign_list_kernel, dim3(((unsigned)k + 255) / 256), dim3(256), 0, s, (const uint32_t*)up, (const uint32_t*)(up + k), (uint32_t)k,
                           sizes_dev, n);
    }
    hipLaunchKernelGGL(cc_relabel_kernel, dim3(eng_blocks(n, 1 << 20)), dim3(256), 0, s, lab_dev, sizes_dev, n);
    ENG_HIP_CLEANUP(e, hipGetLastError());
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));       // the host lists and `up` must outlive the upload and the assign
    cleanup();
    return SABER_OK;
}
