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
    const uint32_t min_vol = min_mask_area > 0 ? (uint32_t)std::min<int64_t>((int64_t)min_mask_area * 10, 0x7fffffff) : 0u;   // utils.py:113
    // a kept component has >= max(min_vol, 1) voxels; isolated voxels of a 26-connected labelling are >= 2 apart in every axis
    const int64_t cap64 = min_vol > 1 ? n / min_vol + 1 : (int64_t)((Z + 1) / 2) * ((H + 1) / 2) * ((W + 1) / 2) + 1;
    const uint32_t cap = (uint32_t)cap64;
    ENG_HIP_CLEANUP(e, hipMalloc(&lab, (size_t)n * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&list, (size_t)cap * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&counter, 4));
    ENG_HIP_CLEANUP(e, hipMemsetAsync(counter, 0, 4, s));
    ENG_HIP_CLEANUP(e, hipMemsetAsync(out_dev, 0, (size_t)n * 4, s));
    const int64_t rows = (int64_t)Z * H;
    const unsigned vox_blocks = eng_blocks(n, 1 << 20);
    ccl_init(planes_dev, lab, nullptr, nullptr, W, rows, s);
    hipLaunchKernelGGL(cc_merge_kernel, dim3(vox_blocks), dim3(256), 0, s, planes_dev, lab, Z, H, W);
    ccl_flatten(lab, n, vox_blocks, s);
    ccl_count(lab, out_dev, W, rows, s);
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
