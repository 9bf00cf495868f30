// Hole filling of mask logits on the device: upstream's fill_holes_in_mask_scores (sam2/utils/misc.py, the step SAM2VideoPredictor runs
// after every single-frame inference when fill_hole_area > 0; upstream needs its connected-components CUDA extension for it).  Per plane:
// the 8-connected components of the background (logit <= 0) are labelled and sized, and every pixel of a component of at most max_area
// pixels takes fill_value (upstream: 0.1).  The fourth consumer of the union-find core of ccl.h, batched over planes.
//
// Kernels, all on the caller's stream, no synchronisation and no allocation:
//   hf_init      one wave per row: a background pixel starts as a child of the first pixel of its x-run (ccl_run_start with the
//                predicate `<= 0`); sizes cleared on the way
//   hf_merge     per background pixel of a row that is not its plane's first: the pixel above, or - when that one is foreground - the two
//                diagonal ones above, guarded by the row's ends.  Rows of different planes never meet, so planes that are adjacent in
//                memory stay apart
//   ccl_flatten  parent <- root
//   ccl_count    pixels per root
//   hf_write     out = sizes[root] <= max_area ? fill_value : in, bit for bit (a pixel reads and writes its own entry: out may be in)
#include "ccl.h"
#include "engine.h"
#include "kernels.h"

// background: value <= 0.0f on the bits (no dependence on the denormal mode): either zero, or a negative number that is not a NaN
__device__ __forceinline__ bool hf_background(uint32_t bits) {
    return (bits << 1) == 0u || ((bits >> 31) != 0u && (bits & 0x7fffffffu) <= 0x7f800000u);
}

__global__ __launch_bounds__(256) void hf_init_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ lab, uint32_t* __restrict__ sizes, int W,
                                                      int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // wave-uniform
    const uint32_t base = (uint32_t)(row * W);                 // fewer than 2^31 pixels in all: indices fit 32 bits
    uint32_t carry = CCL_NONE;
    for (int x0 = 0; x0 < W; x0 += 64) {                       // wave-uniform trip count
        const int x = x0 + lane;
        const uint32_t i = base + (uint32_t)x;
        const uint32_t start = ccl_run_start(x < W && hf_background(in[i]), lane, base + (uint32_t)x0, carry);
        if (x < W) {
            lab[i] = start;
            sizes[i] = 0u;
        }
    }
}

// Entries of `lab` never become CCL_NONE, nor leave it, while merges run: "is background" can be read from it.  A union is left out where
// a neighbour in the same run makes it: the pixel to the left (its own upper neighbour is this pixel's upper-left one) or to the right.
__global__ __launch_bounds__(256) void hf_merge_kernel(uint32_t* lab, int H, int W, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        if (lab[v] == CCL_NONE) continue;
        const int64_t row = v / W;
        if (row % H == 0) continue;                            // a plane's first row: what lies before it belongs to another plane
        const int x = (int)(v - row * W);
        const int64_t u = v - W;
        const bool up = lab[u] != CCL_NONE;
        const bool has_l = x > 0, has_r = x + 1 < W;           // the row's ends: v - 1 / u - 1 and v + 1 / u + 1 are in other rows there
        const bool left = has_l && lab[v - 1] != CCL_NONE, up_l = has_l && lab[u - 1] != CCL_NONE;
        if (up) {
            if (!(left && up_l)) ccl_unite(lab, (uint32_t)v, (uint32_t)u);      // else the left pixel joins the two runs
        } else {
            if (up_l && !left) ccl_unite(lab, (uint32_t)v, (uint32_t)(u - 1));
            if (has_r && lab[u + 1] != CCL_NONE && lab[v + 1] == CCL_NONE) ccl_unite(lab, (uint32_t)v, (uint32_t)(u + 1));
        }
    }
}

void ccl8_merge_planes(uint32_t* lab, int H, int W, int64_t n, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(hf_merge_kernel, dim3(blocks), dim3(256), 0, s, lab, H, W, n);
}

__global__ __launch_bounds__(256) void hf_write_kernel(const uint32_t* in, const uint32_t* __restrict__ lab, const uint32_t* __restrict__ sizes,
                                                       uint32_t max_area, uint32_t fill_bits, uint32_t* out, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const uint32_t r = lab[v];
        out[v] = (r != CCL_NONE && sizes[r] <= max_area) ? fill_bits : in[v];
    }
}

const char* launch_fill_holes(const float* in, int n_planes, int H, int W, int max_area, float fill_value, float* out, void* workspace,
                              size_t workspace_bytes, hipStream_t s) {
    if (n_planes < 1 || H < 1 || W < 1) return "fill_holes: n_planes, H and W must be at least 1";
    if (max_area < 1) return "fill_holes: max_area must be at least 1";
    if (!in || !out || !workspace) return "fill_holes: null pointer";
    const int64_t rows = (int64_t)n_planes * H, n = rows * W;
    if (n >= ((int64_t)1 << 31)) return "fill_holes: 2^31 pixels or more are not supported";
    if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)workspace) & 3u) return "fill_holes: pointers must be 4-byte aligned";
    if (workspace_bytes < (size_t)n * 8) return "fill_holes: the workspace is too small (8 bytes per pixel: n_planes * H * W * 8)";
    uint32_t* lab = (uint32_t*)workspace;
    uint32_t* sizes = lab + n;
    const unsigned row_blocks = (unsigned)((rows + 3) / 4), px_blocks = eng_blocks(n);
    union { float f; uint32_t u; } fill;
    fill.f = fill_value;
    hipLaunchKernelGGL(hf_init_kernel, dim3(row_blocks), dim3(256), 0, s, (const uint32_t*)in, lab, sizes, W, rows);
    if (H > 1) ccl8_merge_planes(lab, H, W, n, px_blocks, s);
    ccl_flatten(lab, n, px_blocks, s);
    ccl_count(lab, sizes, W, rows, s);
    hipLaunchKernelGGL(hf_write_kernel, dim3(px_blocks), dim3(256), 0, s, (const uint32_t*)in, (const uint32_t*)lab, (const uint32_t*)sizes,
                       (uint32_t)max_area, fill.u, (uint32_t*)out, n);
    return nullptr;
}
