// Clean-up of the low-resolution mask logits on the device: upstream's SAM2Transforms.postprocess_masks (sam2/utils/transforms.py, with
// get_connected_components of sam2/utils/misc.py), the step SAM2ImagePredictor(max_hole_area=.., max_sprinkle_area=..) runs on the
// 256 x 256 logits of every _predict call BEFORE they are resized, thresholded and scored - upstream needs its connected-components CUDA
// extension for it.  Per plane x (H x W fp32, H W <= 65 536), threshold t, areas h and s:
//   background = x <= t, foreground = x > t (IEEE: -0 is background at t = 0; a NaN is in neither set, joins nothing, never changes)
//   holes      if h > 0: every pixel of an 8-connected background component of at most h pixels <- fp32(double(t) + 10)
//   sprinkles  if s > 0: every pixel of an 8-connected foreground component of at most s pixels <- fp32(double(t) - 10)
// Both labellings are of the ORIGINAL plane (a small hole inside a small sprinkle ends at t + 10 inside an island at t - 10), both
// comparisons are <=, no component is exempt at the border, every other pixel keeps its bits.
//
// One workgroup of 1024 threads per plane, the whole union-find in LDS (no workspace, whatever the number of planes):
//   par   65 536 x 16 bit  parent of a pixel: a pixel of the SAME polarity and component whose index is not larger (ccl.h's invariants;
//                          both polarities live in the one array - a pixel is only ever united with pixels of its own polarity)
//   fgm / bgm  65 536 bits each: the two polarities (a NaN, and a pixel past the plane's end, is in neither)
// 128 KiB + 16 KiB = 147 456 B of the CU's 160 KiB.  A wave owns the 64-pixel chunks c = wave, wave + 16, ..: lane l is pixel 64 c + l in
// every phase, so what a lane learns about its pixels stays in its registers (one bit per chunk).  Phases, a barrier between them:
//   load     the plane is read once, coalesced, LC_PRE chunks of a wave in flight; ballots make the polarity words; par <- first pixel of the pixel's x-run inside its
//            chunk and row (joined before the first atomic, as ccl_run_start does)
//   merge    per pixel: the left neighbour across a chunk boundary, and the row above as holefill.hip's merge does, with "same polarity"
//            for "background".  A root changes by compare-and-swap of the 32-bit word that holds it (the 16-bit atomicMin of ccl_unite),
//            path halving writes 16 bits of a non-root: entries only ever decrease along their own ancestor chain
//   flatten  par <- root; a lane notes which of its pixels are roots
//   clear    the roots' entries: a root's entry is free now (its pixel's root is the pixel itself) and becomes the component's counter
//   count    pixels per root EXCEPT the root itself, so the 65 536 pixels of a plane-wide component count 65 535 and fit 16 bits; runs of
//            equal roots inside a chunk are summed by ballot and added with one 32-bit LDS atomic, shifted to the entry's half (the
//            lower half cannot carry: its final value fits)
//   write    size - 1 < area decides; only changed pixels are stored
// Min-index roots and exact counts: every decision is the same whatever order the merges ran in, two calls give the same bytes.
#include "engine.h"
#include "kernels.h"

#define LC_THREADS 1024
#define LC_WAVES (LC_THREADS / 64)
#define LC_PRE 8              // chunks of a wave in flight in the load phase
#define LC_MAX_PIXELS 65536
#define LC_NONE 0xffffffffu

typedef uint16_t __attribute__((may_alias)) lc_u16;
typedef uint32_t __attribute__((may_alias)) lc_u32;

// total order of the non-NaN floats on their bits, -0 = +0 (no dependence on the denormal mode)
__device__ __forceinline__ uint32_t lc_key(uint32_t bits) {
    if ((bits << 1) == 0u) bits = 0u;
    return (bits >> 31) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ bool lc_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }

__device__ __forceinline__ uint32_t lc_find(volatile lc_u16* par, uint32_t x) {
    uint32_t p = par[x];
    while (p != x) {
        const uint32_t g = par[p];
        if (g != p) par[x] = (uint16_t)g;      // path halving: only entries of non-roots are written, and only with an ancestor
        x = p;
        p = g;
    }
    return x;
}
__device__ __forceinline__ void lc_unite(volatile lc_u16* par, uint32_t a, uint32_t b) {
    lc_u32* par32 = (lc_u32*)par;
    while (true) {
        a = lc_find(par, a);
        b = lc_find(par, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }      // hang the larger root under the smaller one
        lc_u32* word = par32 + (a >> 1);
        const uint32_t sh = (a & 1u) * 16u;
        uint32_t old = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (true) {
            const uint32_t cur = (old >> sh) & 0xffffu;
            if (cur != a) { a = cur; break; }                   // somebody re-parented a meanwhile: continue from there
            const uint32_t neu = (old & ~(0xffffu << sh)) | (b << sh);
            const uint32_t prev = atomicCAS(word, old, neu);
            if (prev == old) return;
            old = prev;                                         // the other half of the word changed, or a did
        }
    }
}

// is pixel u in the polarity whose words are m
__device__ __forceinline__ bool lc_in(const lc_u32* m, uint32_t u) { return (m[u >> 5] >> (u & 31u)) & 1u; }

__global__ __launch_bounds__(LC_THREADS) void lc_clean_kernel(float* __restrict__ planes, const int* __restrict__ idx, const uint8_t* __restrict__ pass, int W, uint32_t n,
                                                              uint32_t thr_bits, uint32_t hole_area, uint32_t sprinkle_area, uint32_t hole_bits, uint32_t sprinkle_bits) {
    __shared__ uint32_t par_words[LC_MAX_PIXELS / 2];
    __shared__ unsigned long long fgm[LC_MAX_PIXELS / 64], bgm[LC_MAX_PIXELS / 64];
    const uint32_t k = blockIdx.x;
    if (pass && !pass[k]) return;                               // block-uniform: in front of every barrier
    uint32_t* px = reinterpret_cast<uint32_t*>(planes) + (size_t)(idx ? idx[k] : (int)k) * n;
    volatile lc_u16* par = (volatile lc_u16*)par_words;
    lc_u32* par32 = (lc_u32*)par_words;
    const lc_u16* lab = (const lc_u16*)par_words;               // the phases in which no entry they read changes
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t nch = (n + 63u) >> 6;                        // chunks; every loop over them has a wave-uniform trip count
    const uint32_t uW = (uint32_t)W;
    const bool pow2 = (uW & (uW - 1u)) == 0u;                   // the generator's 256: no division per pixel
    const bool thr_ok = !lc_nan(thr_bits);
    const uint32_t tkey = lc_key(thr_bits);
    const unsigned long long below = (2ull << lane) - 1ull;    // lanes 0 .. lane
    unsigned long long fgb = 0ull, bgb = 0ull, roots = 0ull;    // bit i: the lane's pixel of its i-th chunk is foreground / background / a root

    // ---- load: LC_PRE chunks of the wave in flight at a time (one plane per CU: nothing else hides the latency of HBM)
    for (uint32_t c0 = wave, i0 = 0; c0 < nch; c0 += LC_WAVES * LC_PRE, i0 += LC_PRE) {
        uint32_t val[LC_PRE];
#pragma unroll
        for (uint32_t j = 0; j < LC_PRE; ++j) {
            const uint32_t v = (c0 + j * LC_WAVES) * 64u + lane;
            val[j] = v < n ? px[v] : 0x7fc00000u;              // (a chunk past the last one starts at or past n)
        }
#pragma unroll
        for (uint32_t j = 0; j < LC_PRE; ++j) {
            const uint32_t c = c0 + j * LC_WAVES;
            if (c < nch) {                                      // wave-uniform
                const uint32_t v = c * 64u + lane;
                const bool in = v < n;
                const bool valid = in && thr_ok && !lc_nan(val[j]);
                const bool fg = valid && lc_key(val[j]) > tkey, bg = valid && !fg;
                const unsigned long long f = __ballot(fg), b = __ballot(bg), rs = __ballot(in && (pow2 ? (v & (uW - 1u)) : v % uW) == 0u);
                if (lane == 0) { fgm[c] = f; bgm[c] = b; }
                fgb |= (unsigned long long)fg << (i0 + j);
                bgb |= (unsigned long long)bg << (i0 + j);
                if (in) {
                    // a run starts at the chunk's first lane, at a row's first pixel and behind a pixel of another polarity
                    const unsigned long long mine = fg ? f : b;
                    const unsigned long long stop = (~mine << 1) | rs | 1ull;
                    const uint32_t start = 63u - (uint32_t)__clzll((long long)(stop & below));
                    par[v] = (uint16_t)(valid ? c * 64u + start : v);
                }
            }
        }
    }
    __syncthreads();
    // ---- merge
    for (uint32_t c = wave, i = 0; c < nch; c += LC_WAVES, ++i) {
        const uint32_t v = c * 64u + lane;
        const bool fg = (fgb >> i) & 1ull, bg = (bgb >> i) & 1ull;
        if (!(fg || bg)) continue;
        const lc_u32* m = (const lc_u32*)(fg ? fgm : bgm);
        const uint32_t x = pow2 ? (v & (uW - 1u)) : v % uW;
        const bool has_l = x > 0u, has_r = x + 1u < uW;         // the row's ends: v - 1 / u - 1 and v + 1 / u + 1 are in other rows there
        const bool left = has_l && lc_in(m, v - 1u);
        if (lane == 0 && left) lc_unite(par, v, v - 1u);        // a run that crosses the chunk's boundary
        if (v < uW) continue;                                   // the plane's first row
        const uint32_t u = v - uW;
        const bool up_l = has_l && lc_in(m, u - 1u);
        if (lc_in(m, u)) {
            if (!(left && up_l)) lc_unite(par, v, u);           // else the left pixel joins the two runs
        } else {
            if (up_l && !left) lc_unite(par, v, u - 1u);
            if (has_r && lc_in(m, u + 1u) && !lc_in(m, v + 1u)) lc_unite(par, v, u + 1u);
        }
    }
    __syncthreads();
    // ---- flatten (a chase that meets an entry already flattened reads an ancestor all the same); a root's entry does not change here
    for (uint32_t c = wave, i = 0; c < nch; c += LC_WAVES, ++i) {
        const uint32_t v = c * 64u + lane;
        if (!(((fgb | bgb) >> i) & 1ull)) continue;
        uint32_t p = par[v];
        if (p == v) { roots |= 1ull << i; continue; }
        while (true) {
            const uint32_t g = par[p];
            if (g == p) break;
            p = g;
        }
        par[v] = (uint16_t)p;
    }
    __syncthreads();                                            // every entry read as a label before one becomes a counter
    for (uint32_t c = wave, i = 0; c < nch; c += LC_WAVES, ++i)
        if ((roots >> i) & 1ull) par[c * 64u + lane] = 0;
    __syncthreads();
    // ---- count: size - 1 at the root's entry
    for (uint32_t c = wave, i = 0; c < nch; c += LC_WAVES, ++i) {
        const uint32_t v = c * 64u + lane;
        const bool member = (((fgb | bgb) & ~roots) >> i) & 1ull;
        const uint32_t key = member ? (uint32_t)lab[v] : LC_NONE;
        const uint32_t prev = __shfl_up(key, 1, 64);
        const bool head = lane == 0 || key != prev;
        const unsigned long long heads = __ballot(head);
        const unsigned long long rest = lane == 63u ? 0ull : heads >> (lane + 1u);
        const uint32_t len = rest ? (uint32_t)__ffsll((long long)rest) : 64u - lane;      // lanes up to the next head
        if (head && key != LC_NONE) atomicAdd(par32 + (key >> 1), len << ((key & 1u) * 16u));
    }
    __syncthreads();
    // ---- write
    for (uint32_t c = wave, i = 0; c < nch; c += LC_WAVES, ++i) {
        const uint32_t v = c * 64u + lane;
        const bool fg = (fgb >> i) & 1ull, bg = (bgb >> i) & 1ull;
        const uint32_t area = fg ? sprinkle_area : bg ? hole_area : 0u;
        if (area == 0u) continue;
        const uint32_t r = ((roots >> i) & 1ull) ? v : (uint32_t)lab[v];
        if ((uint32_t)lab[r] < area) px[v] = fg ? sprinkle_bits : hole_bits;
    }
}

const char* launch_clean_lowres(float* planes, const int* idx, const uint8_t* pass, int n, int H, int W, float thr, int max_hole_area, int max_sprinkle_area,
                                hipStream_t s) {
    if (!planes) return "clean_lowres: null planes";
    if (n < 0) return "clean_lowres: n must be at least 0";
    if (H < 1 || W < 1 || (int64_t)H * W > LC_MAX_PIXELS) return "clean_lowres: planes of 1 to 65536 pixels (H, W at least 1)";
    if (max_hole_area < 0 || max_hole_area > 65535 || max_sprinkle_area < 0 || max_sprinkle_area > 65535)
        return "clean_lowres: max_hole_area and max_sprinkle_area must be 0 to 65535";
    if ((uintptr_t)planes & 3u) return "clean_lowres: planes must be 4-byte aligned";
    if (n == 0 || (max_hole_area == 0 && max_sprinkle_area == 0)) return nullptr;
    union { float f; uint32_t u; } t, hi, lo;
    t.f = thr;
    hi.f = (float)((double)thr + 10.0);
    lo.f = (float)((double)thr - 10.0);
    hipLaunchKernelGGL(lc_clean_kernel, dim3((unsigned)n), dim3(LC_THREADS), 0, s, planes, idx, pass, W, (uint32_t)(H * W), t.u, (uint32_t)max_hole_area,
                       (uint32_t)max_sprinkle_area, hi.u, lo.u);
    return nullptr;
}
