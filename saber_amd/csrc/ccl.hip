// The labelling kernels that are the same for every consumer of ccl.h: run-start initialisation, flatten, per-root voxel count.
// The merge kernels stay with their consumers (three different neighbour rules).
#include "ccl.h"

// one wave per row: every foreground voxel starts as a child of the first voxel of its x-run
template <typename T>
__global__ __launch_bounds__(256) void ccl_init_kernel(const T* __restrict__ m, uint32_t* __restrict__ lab, uint32_t* __restrict__ sizes,
                                                       uint32_t* __restrict__ ov, int W, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // wave-uniform
    const uint32_t base = (uint32_t)(row * W);                 // every consumer rejects volumes of 2^31 voxels or more: indices fit 32 bits,
    uint32_t carry = CCL_NONE;                                 // and one offset register serves the three arrays
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const uint32_t i = base + (uint32_t)x;
        const uint32_t start = ccl_run_start(x < W && m[i] != 0, lane, base + (uint32_t)x0, carry);
        if (x < W) {
            lab[i] = start;
            if (sizes) sizes[i] = 0u;
            if (ov) ov[i] = 0u;
        }
    }
}

__global__ __launch_bounds__(256) void ccl_flatten_kernel(uint32_t* __restrict__ lab, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const uint32_t p = lab[v];
        if (p != CCL_NONE) lab[v] = ccl_root(lab, p);
    }
}

// one wave per row.  Consecutive foreground voxels of a row share their root, so an x-run contributes one atomic per 64-voxel chunk -
// except the runs of the row's LEADING root, which are summed with a ballot and carried from chunk to chunk (pend_root / pend_cnt,
// wave-uniform) until another root takes the lead or the row ends.  The leading root is the carried one while it still occurs in the
// chunk, else the root of the chunk's first foreground voxel: a component that fills most of a row (the background of a mask, cut into
// many runs by specks) then costs the row one atomic instead of one per run, all of which would meet at one address.
__global__ __launch_bounds__(256) void ccl_count_kernel(const uint32_t* __restrict__ lab, uint32_t* __restrict__ sizes, int W, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // wave-uniform
    const int64_t base = row * W;
    uint32_t pend_root = CCL_NONE, pend_cnt = 0u;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const uint32_t r = x < W ? lab[base + x] : CCL_NONE;
        const bool fg = r != CCL_NONE;
        const unsigned long long mask = __ballot(fg);
        if (mask == 0ull) continue;                            // wave-uniform
        uint32_t lead = pend_root;
        if (lead == CCL_NONE || __ballot(r == lead) == 0ull) lead = __shfl(r, __ffsll((long long)mask) - 1, 64);
        const unsigned long long lead_mask = __ballot(r == lead);
        const bool head = fg && r != lead && (lane == 0 || !((mask >> (lane - 1)) & 1ull));
        if (head) {
            const unsigned long long above_bg = ~mask & ~((2ull << lane) - 1ull);      // background lanes above this one
            const int end = above_bg ? __ffsll((long long)above_bg) - 1 : 64;           // first background lane after the run
            atomicAdd(&sizes[r], (uint32_t)(end - lane));
        }
        if (lead != pend_root) {
            if (lane == 0 && pend_root != CCL_NONE) atomicAdd(&sizes[pend_root], pend_cnt);
            pend_root = lead;
            pend_cnt = 0u;
        }
        pend_cnt += (uint32_t)__popcll(lead_mask);
    }
    if (lane == 0 && pend_root != CCL_NONE) atomicAdd(&sizes[pend_root], pend_cnt);
}

template <typename T>
void ccl_init(const T* fg, uint32_t* lab, uint32_t* sizes_or_null, uint32_t* ov_or_null, int W, int64_t rows, hipStream_t s) {
    hipLaunchKernelGGL(ccl_init_kernel<T>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, fg, lab, sizes_or_null, ov_or_null, W, rows);
}
template void ccl_init<uint16_t>(const uint16_t*, uint32_t*, uint32_t*, uint32_t*, int, int64_t, hipStream_t);      // separate_masks
template void ccl_init<uint8_t>(const uint8_t*, uint32_t*, uint32_t*, uint32_t*, int, int64_t, hipStream_t);        // components6

void ccl_flatten(uint32_t* lab, int64_t n, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3(blocks), dim3(256), 0, s, lab, n);
}

void ccl_count(const uint32_t* lab, uint32_t* sizes, int W, int64_t rows, hipStream_t s) {
    hipLaunchKernelGGL(ccl_count_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, lab, sizes, W, rows);
}
