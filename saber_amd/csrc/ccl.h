// Connected-component labelling core shared by cc3d.hip (26-connected, 3-D), morph3d.hip (6-connected, 3-D) and consensus2d.hip
// (4-connected, 2-D): union-find with min-index roots.
//
// `lab` holds one uint32 per voxel: CCL_NONE for background, else the index of a voxel of the same component that is not larger
// than the voxel's own (its parent); a voxel that is its own parent is a root.  Two roots are only ever joined by hanging the larger
// index under the smaller one, so when the merges are done a component's root IS its smallest index: its first voxel in C-order
// scan.  scipy.ndimage.label numbers components in the order its scan meets them, which is the ascending order of exactly these
// first voxels; rank the roots by index and the numbering is scipy's, whatever order the device ran the merges in.
//   1. init     one wave per row (or row segment): every foreground voxel starts as a child of the first voxel of its x-run
//               (ccl_run_start), so x-neighbours are joined before the first atomic
//   2. merge    the consumer's own kernel: ccl_unite(v, u) for the neighbours u that precede v in scan order, as its connectivity says
//   3. flatten  parent <- root (ccl_root), after which `lab` is read-only
//   4. count    voxels per root, at the root's index in `sizes` (one atomic per x-run and 64-voxel chunk; the runs of a row's leading
//               root are summed and carried along the row: one atomic per row for a component that fills most of it)
// What makes it safe without locks: a root's entry changes by atomicMin alone (ccl_unite), path halving writes only entries of
// non-roots and only with an ancestor (ccl_find), so every entry only ever decreases along its own ancestor chain and a chase always
// ends at a root.  The ballots and shuffles of the row kernels need whole waves: early exits in front of them are wave-uniform.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CCL_NONE 0xffffffffu

__device__ __forceinline__ uint32_t ccl_find(uint32_t* lab, uint32_t x) {
    uint32_t p = lab[x];
    while (p != x) {
        const uint32_t g = lab[p];
        if (g != p) lab[x] = g;      // path halving: only non-root entries are written, roots change by atomicMin alone
        x = p;
        p = g;
    }
    return x;
}
__device__ __forceinline__ void ccl_unite(uint32_t* lab, uint32_t a, uint32_t b) {
    while (true) {
        a = ccl_find(lab, a);
        b = ccl_find(lab, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }      // hang the larger root under the smaller one
        const uint32_t old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;                                               // somebody re-parented a meanwhile: continue from there
    }
}

// Index of the first voxel of this lane's x-run, CCL_NONE for a background lane.  The wave holds 64 consecutive voxels of a row,
// lane 0 the one with index chunk0.  carry: start of the run that reaches the previous chunk's last voxel (CCL_NONE at a row's or
// segment's first chunk); updated from lane 63 for the next chunk, CCL_NONE again when that voxel is background or past the row.
// EVERY lane of the wave must call it (ballot + shuffle): lanes past the row's end pass fg = false.
__device__ __forceinline__ uint32_t ccl_run_start(bool fg, int lane, uint32_t chunk0, uint32_t& carry) {
    const unsigned long long mask = __ballot(fg);
    uint32_t start = CCL_NONE;
    if (fg) {
        const unsigned long long below_bg = ~mask & ((1ull << lane) - 1ull);
        if (below_bg == 0ull) start = carry != CCL_NONE ? carry : chunk0;
        else start = chunk0 + (uint32_t)(64 - __clzll((long long)below_bg));      // the lane after the last background lane below me
    }
    carry = __shfl(start, 63, 64);
    return start;
}

// read-only chase from a parent p to its root (the flatten kernels: no merge runs beside them)
__device__ __forceinline__ uint32_t ccl_root(const uint32_t* lab, uint32_t p) {
    while (true) {
        const uint32_t g = lab[p];
        if (g == p) return p;
        p = g;
    }
}

// ---- launchers of the kernels every consumer shares (ccl.hip); all of them only enqueue, the caller checks hipGetLastError
// lab <- run starts of the rows of `fg` (foreground = non-zero); sizes / ov, where given, are cleared on the way (n entries each)
template <typename T>
void ccl_init(const T* fg, uint32_t* lab, uint32_t* sizes_or_null, uint32_t* ov_or_null, int W, int64_t rows, hipStream_t s);
// lab[v] <- root(v); `blocks` of 256 threads stride over the n voxels (the caller's cap on its voxel grids)
void ccl_flatten(uint32_t* lab, int64_t n, unsigned blocks, hipStream_t s);
// sizes[root] += voxels, for a flattened lab and sizes cleared beforehand
void ccl_count(const uint32_t* lab, uint32_t* sizes, int W, int64_t rows, hipStream_t s);
