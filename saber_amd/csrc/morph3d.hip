// Organelle / membrane refinement on the device: 3-D ball morphology on bit-packed rows, 6-connected components, and the pipeline
// that drives them.  Replaces saber.analysis.refine_membranes.OrganelleMembraneFilter.run (saber/analysis/refine_membranes.py:445-547)
// with _process_organelle_batch (:335-443) and the helpers under it: _trim_edges (:119-134), _remove_small_objects (:136-159),
// _keep_surface_membranes_only (:161-199), _remove_small_membrane_components (:201-224), _get_largest_component (:226-249),
// _get_organelle_roi (:251-272), _torch_erosion_3d / _torch_dilation_3d / _morphological_opening (:274-333).
//
// The reference dilates and erodes with a dense fp32 conv3d of (2r+1)^3 taps, labels on the host with scipy.ndimage.label, clones the
// volume per organelle and synchronises after every step.  Here everything is integer work on 0/1 data, so the results are exact:
//   mo_pack / mo_unpack   a (Z,H,W) ROI <-> rows bit-packed along x (bit i of word w = voxel 32 w + i), rows padded to whole words
//   mo_ball<ERODE>        a ball of radius r is a union of x-runs of half-length half(dz,dy) = floor(sqrt(r^2 - dz^2 - dy^2)).  With
//                         A[k] = OR of the rows whose half >= k, the dilation is OR_k (A[k] << k | A[k] >> k): the (dz,dy) offsets are
//                         visited in descending half, so A is one running accumulator (3 words: left neighbour, centre, right neighbour)
//                         and every offset costs 3 LDS reads + 3 ORs, every k two funnel shifts.  Erosion is the dual with AND; voxels
//                         outside the volume are 0 for both.  A block owns TY rows x TW words and walks z: a ring of 2r+1 packed
//                         planes (with a halo of r rows and one word) lives in LDS, each step loads one new plane.
//   cc6_*                 the union-find with min-index roots of ccl.h, 6-connectivity: x-neighbours through the runs of ccl_init,
//                         then (z,y-1,x) and (z-1,y,x) in cc6_merge.  Two consumers, both without a host round trip: "zero the
//                         components below min_size" and "keep the largest, the first in raster order on ties" (one 64-bit atomicMax
//                         over the roots of size << 32 | ~root).
//   label_max_host / label_stats_host   largest label, voxel count + bounding box per organelle label on the planes that hold membrane (smooth3d.hip)
//   small kernels         edge trim, per-z membrane presence, byte OR / AND, population count, the 3x3x3 organelle boundary of the
//                         surface test (inside cc6_overlap), scatter into the two label maps, expansion of stored pairs into planes.
// Host synchronisations of one saber_refine_membranes call: 3 (largest label; per-label statistics; per-organelle flags at the end),
// whatever the number of labels or voxels.  The reference's `.sum() == 0` tests are device-side counters.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ccl.h"
#include "common.h"
#include "engine.h"

#define MO_MAX_R 16
#define MO_ZC 16                 // output planes per block of mo_ball (the ring is refilled per chunk: 2r planes of halo)
#define MO_MAX_LABEL (1u << 22)
#define MO_LDS_LIMIT (150 * 1024)

// ------------------------------------------------------------------------------------------------ pack / unpack
// One wave per 64 voxels of a row.  LABEL: voxel == label and the plane's z flag is set; otherwise voxel != 0.
template <typename T, bool LABEL>
__global__ __launch_bounds__(256) void mo_pack_kernel(const T* __restrict__ src, int64_t sz, int64_t sy, uint32_t label,
                                                      const uint8_t* __restrict__ zflag, int dy, int64_t rows, int dx, int WW,
                                                      uint32_t* __restrict__ out) {
    const int chunks = (dx + 63) / 64;
    const int64_t piece = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (piece >= rows * chunks) return;                        // wave-uniform
    const int64_t row = piece / chunks;
    const int c = (int)(piece % chunks), lane = threadIdx.x & 63;
    const int z = (int)(row / dy), y = (int)(row % dy);
    const int x = c * 64 + lane;
    bool bit = false;
    if (x < dx) {
        const T v = src[z * sz + y * sy + x];
        bit = LABEL ? ((uint32_t)v == label && zflag[z] != 0) : (v != 0);
    }
    const unsigned long long m = __ballot(bit);
    if (lane == 0) out[row * WW + 2 * c] = (uint32_t)m;
    if (lane == 1 && 2 * c + 1 < WW) out[row * WW + 2 * c + 1] = (uint32_t)(m >> 32);
}

// out = bits of a (AND b when given); when `counter` is given and *counter == 0 the bits of `alt` are taken instead (the
// "opening left nothing: use the unopened mask" fall-back of refine_membranes.py:414-416)
__global__ __launch_bounds__(256) void mo_unpack_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                        const uint32_t* __restrict__ alt, const uint32_t* __restrict__ counter, int64_t rows,
                                                        int dx, int WW, uint8_t* __restrict__ out) {
    const uint32_t* p = (counter && *counter == 0u) ? alt : a;
    const int64_t n = rows * dx;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const int64_t row = v / dx;
        const int x = (int)(v % dx);
        uint32_t w = p[row * WW + (x >> 5)];
        if (b) w &= b[row * WW + (x >> 5)];
        out[v] = (uint8_t)((w >> (x & 31)) & 1u);
    }
}

__global__ __launch_bounds__(256) void mo_popcount_kernel(const uint32_t* __restrict__ a, int64_t words, uint32_t* __restrict__ counter) {
    uint32_t c = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) c += (uint32_t)__popc(a[i]);
    c = wave_sum_u32(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(counter, c);
}

// ------------------------------------------------------------------------------------------------ ball dilation / erosion
// tab: [0 .. r+1] first entry of the group with half = r - j (tab[r+1] = number of entries), then the entries
// ((dz + r) << 16 | (dy + r)) in descending half.
template <bool ERODE>
__global__ __launch_bounds__(256) void mo_ball_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int Z, int H, int WW, int W,
                                                      int r, int TW, const int* __restrict__ tab) {
    extern __shared__ uint32_t mo_lds[];
    const int TY = 256 / TW, TWH = TW + 2, TYH = TY + 2 * r, D = 2 * r + 1;
    const int plane = TYH * TWH;
    const int tw = threadIdx.x % TW, ty = threadIdx.x / TW;
    const int wx0 = blockIdx.x * TW, y0 = blockIdx.y * TY;
    const int zc0 = blockIdx.z * MO_ZC, zc1 = min(Z, zc0 + MO_ZC);
    auto load_plane = [&](int p) {                             // plane p (zeros when outside the volume) -> ring slot (p + r) % D
        uint32_t* dst = mo_lds + ((p + r) % D) * plane;
        const bool zin = p >= 0 && p < Z;
        for (int i = threadIdx.x; i < plane; i += 256) {
            const int yy = y0 - r + i / TWH, ww = wx0 - 1 + i % TWH;
            uint32_t v = 0u;
            if (zin && yy >= 0 && yy < H && ww >= 0 && ww < WW) v = in[((int64_t)p * H + yy) * WW + ww];
            dst[i] = v;
        }
    };
    for (int p = zc0 - r; p < zc0 + r; ++p) load_plane(p);
    const int* ent = tab + (r + 2);
    const bool live = (y0 + ty < H) && (wx0 + tw < WW);
    const uint32_t tail = (wx0 + tw == WW - 1 && (W & 31)) ? ((1u << (W & 31)) - 1u) : 0xffffffffu;   // bits past the row's end stay 0
    const uint32_t ident = ERODE ? 0xffffffffu : 0u;
    for (int z = zc0; z < zc1; ++z) {
        load_plane(z + r);
        __syncthreads();
        if (live) {
            const int zm = z % D;                              // ring slot of plane z - r
            const uint32_t* base = mo_lds + ty * TWH + tw + 1;
            uint32_t al = ident, ac = ident, ar = ident, res = ident;
            for (int h = r; h >= 0; --h) {
                const int e1 = tab[r - h + 1];
                for (int i = tab[r - h]; i < e1; ++i) {
                    const int en = ent[i];
                    int s = zm + (en >> 16);
                    if (s >= D) s -= D;
                    const uint32_t* q = base + s * plane + (en & 0xffff) * TWH;
                    if (ERODE) { al &= q[-1]; ac &= q[0]; ar &= q[1]; }
                    else { al |= q[-1]; ac |= q[0]; ar |= q[1]; }
                }
                uint32_t t = ac;
                if (h > 0) {
                    const uint32_t up = (ac << h) | (al >> (32 - h)), dn = (ac >> h) | (ar << (32 - h));
                    t = ERODE ? (up & dn) : (up | dn);
                }
                res = ERODE ? (res & t) : (res | t);
            }
            out[((int64_t)z * H + y0 + ty) * WW + wx0 + tw] = res & tail;
        }
        __syncthreads();                                       // the next step overwrites the slot of plane z - r
    }
}

// ------------------------------------------------------------------------------------------------ 6-connected components
__global__ __launch_bounds__(256) void cc6_merge_kernel(const uint8_t* __restrict__ m, uint32_t* __restrict__ lab, int Z, int H, int W) {
    const int64_t n = (int64_t)Z * H * W;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        if (m[v] == 0) continue;
        const int64_t row = v / W;
        const int y = (int)(row % H), z = (int)(row / H);
        if (y > 0 && m[v - W] != 0) ccl_unite(lab, (uint32_t)v, (uint32_t)(v - W));
        if (z > 0 && m[v - (int64_t)H * W] != 0) ccl_unite(lab, (uint32_t)v, (uint32_t)(v - (int64_t)H * W));
    }
}

// surface test (refine_membranes.py:161-199): ov[root] = voxels of the component on the organelle's boundary, the organelle voxels
// with a zero (or the ROI's outside) among their 26 neighbours
__global__ __launch_bounds__(256) void cc6_overlap_kernel(const uint32_t* __restrict__ lab, const uint8_t* __restrict__ org, uint32_t* __restrict__ ov,
                                                          int Z, int H, int W) {
    const int64_t n = (int64_t)Z * H * W;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const uint32_t r = lab[v];
        if (r == CCL_NONE || org[v] == 0) continue;
        const int x = (int)(v % W);
        const int64_t row = v / W;
        const int y = (int)(row % H), z = (int)(row / H);
        bool inner = x > 0 && x + 1 < W && y > 0 && y + 1 < H && z > 0 && z + 1 < Z;
        for (int dz = -1; inner && dz <= 1; ++dz)
            for (int dy = -1; inner && dy <= 1; ++dy) {
                const uint8_t* p = org + v + ((int64_t)dz * H + dy) * W;
                inner = p[-1] != 0 && p[0] != 0 && p[1] != 0;
            }
        if (!inner) atomicAdd(&ov[r], 1u);
    }
}

// mode 0: a component stays when it has >= min_size voxels (and, with ov, more than a tenth of them on the boundary)
__global__ __launch_bounds__(256) void cc6_filter_kernel(const uint8_t* m, const uint32_t* __restrict__ lab, const uint32_t* __restrict__ sizes,
                                                         const uint32_t* __restrict__ ov, uint32_t min_size, uint8_t* out, int64_t n,
                                                         uint32_t* __restrict__ kept_voxels, uint32_t* __restrict__ kept_comps) {
    uint32_t kv = 0, kc = 0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const uint32_t r = lab[v];
        uint8_t o = 0;
        if (r != CCL_NONE) {
            const uint32_t sz = sizes[r];
            const bool keep = sz >= min_size && (!ov || (uint64_t)ov[r] * 10u > (uint64_t)sz);     // overlap / size > 0.1
            if (keep) { o = m[v]; ++kv; if (r == (uint32_t)v) ++kc; }
        }
        out[v] = o;
    }
    kv = wave_sum_u32(kv);
    kc = wave_sum_u32(kc);
    if ((threadIdx.x & 63) == 0) {
        if (kept_voxels && kv) atomicAdd(kept_voxels, kv);
        if (kept_comps && kc) atomicAdd(kept_comps, kc);
    }
}

// mode 1: best = max over the roots of (size << 32 | ~root): the largest component, the smallest first voxel on ties
__global__ __launch_bounds__(256) void cc6_best_kernel(const uint32_t* __restrict__ lab, const uint32_t* __restrict__ sizes, int64_t n,
                                                       unsigned long long* __restrict__ best, uint32_t* __restrict__ comps) {
    unsigned long long b = 0ull;
    uint32_t kc = 0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        if (lab[v] != (uint32_t)v) continue;
        const unsigned long long key = ((unsigned long long)sizes[v] << 32) | (unsigned long long)(0xffffffffu - (uint32_t)v);
        b = key > b ? key : b;
        ++kc;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)b, o, 64);
        b = other > b ? other : b;
        kc += (uint32_t)__shfl_xor((int)kc, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (b) atomicMax(best, b);
        if (comps && kc) atomicAdd(comps, kc);
    }
}

__global__ __launch_bounds__(256) void cc6_largest_kernel(const uint8_t* m, const uint32_t* __restrict__ lab,
                                                          const unsigned long long* __restrict__ best, uint8_t* out, int64_t n) {
    const unsigned long long b = *best;
    const uint32_t root = 0xffffffffu - (uint32_t)(b & 0xffffffffull);
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256)
        out[v] = (b != 0ull && lab[v] == root) ? m[v] : (uint8_t)0;
}

// ------------------------------------------------------------------------------------------------ element-wise kernels
// _trim_edges (refine_membranes.py:119-134): out = 1 where the membrane is set inside the trimmed box.  `mask[t:-t]` is empty for
// t = 0, so a zero trim (like one >= dim // 2) leaves nothing: the host passes an empty box then.
__global__ __launch_bounds__(256) void mo_trim_kernel(const uint8_t* __restrict__ mem, uint8_t* __restrict__ out, int Z, int H, int W, int z0, int z1,
                                                      int y0, int y1, int x0, int x1) {
    const int64_t n = (int64_t)Z * H * W;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const int x = (int)(v % W);
        const int64_t row = v / W;
        const int y = (int)(row % H), z = (int)(row / H);
        out[v] = (mem[v] != 0 && z >= z0 && z < z1 && y >= y0 && y < y1 && x >= x0 && x < x1) ? 1 : 0;
    }
}

// zflag[z] = 1 when plane z of the cleaned membrane holds a voxel (every writer stores the same value)
__global__ __launch_bounds__(256) void mo_zpresence_kernel(const uint8_t* __restrict__ m, int64_t plane, uint8_t* __restrict__ zflag) {
    const uint8_t* p = m + (int64_t)blockIdx.y * plane;
    bool any = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < plane && !any; i += (int64_t)gridDim.x * 256) any = p[i] != 0;
    if (__ballot(any) && (threadIdx.x & 63) == 0) zflag[blockIdx.y] = 1;
}

__global__ __launch_bounds__(256) void mo_bytes_op_kernel(const uint8_t* a, const uint8_t* b, int op_and, uint8_t* out,
                                                          int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const bool x = a[v] != 0, y = b[v] != 0;
        out[v] = (op_and ? (x && y) : (x || y)) ? 1 : 0;
    }
}

// a finished pair into the two label maps (refine_membranes.py:433-442 + convert_to_3d_labels :549-573): launches follow each other in
// ascending label order on one stream, so a later organelle overwrites an earlier one exactly as a later plane of the 4-D stack does.
// Nothing is written when the organelle was dropped (*kept == 0: no membrane left after cleaning).
template <typename T>
__global__ __launch_bounds__(256) void mo_scatter_kernel(const uint8_t* __restrict__ org, const uint8_t* __restrict__ mem, const uint32_t* __restrict__ kept,
                                                         T value, int dz, int dy, int dx, int H, int W, int z0, int y0, int x0, T* __restrict__ org_out,
                                                         T* __restrict__ mem_out) {
    if (*kept == 0u) return;
    const int64_t n = (int64_t)dz * dy * dx;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const int x = (int)(v % dx);
        const int64_t row = v / dx;
        const int y = (int)(row % dy), z = (int)(row / dy);
        const int64_t g = ((int64_t)(z0 + z) * H + (y0 + y)) * W + x0 + x;
        if (org[v]) org_out[g] = value;
        if (mem[v]) mem_out[g] = value;
    }
}

// stored packed bits of one pair -> its dense plane of the 4-D stack (the plane is zero already)
template <typename T>
__global__ __launch_bounds__(256) void mo_expand_kernel(const uint32_t* __restrict__ bits, T value, int dz, int dy, int dx, int WW, int H, int W, int z0,
                                                        int y0, int x0, T* __restrict__ plane) {
    const int64_t n = (int64_t)dz * dy * dx;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const int x = (int)(v % dx);
        const int64_t row = v / dx;
        if ((bits[row * WW + (x >> 5)] >> (x & 31)) & 1u) {
            const int y = (int)(row % dy), z = (int)(row / dy);
            plane[((int64_t)(z0 + z) * H + (y0 + y)) * W + x0 + x] = value;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
namespace {
struct MoPair {
    uint32_t label;
    int z0, y0, x0, dz, dy, dx;
    size_t off_org, off_mem;     // first word of the packed organelle / membrane bits in MoState::bits
};

// what a handle keeps between calls: the ball tables and the last saber_refine_membranes call's pairs
struct MoState {
    int* tab_dev[MO_MAX_R + 1] = {};
    std::vector<int> tab_host[MO_MAX_R + 1];
    uint32_t* bits = nullptr;
    std::vector<MoPair> pairs;
    int Z = 0, H = 0, W = 0;
};

MoState* mo_state(saber_engine* e) {
    if (!e->refine_state) e->refine_state = new MoState();
    return (MoState*)e->refine_state;
}

// the (dz,dy) offsets of the ball in descending half-length of their x-run
hipError_t mo_ball_table(MoState* S, int r, hipStream_t s, const int** out) {
    if (!S->tab_dev[r]) {
        std::vector<int>& t = S->tab_host[r];
        t.assign(r + 2, 0);
        for (int h = r; h >= 0; --h) {
            t[r - h] = (int)t.size() - (r + 2);
            for (int dz = -r; dz <= r; ++dz)
                for (int dy = -r; dy <= r; ++dy) {
                    const int rem = r * r - dz * dz - dy * dy;
                    if (rem < 0) continue;
                    int half = 0;
                    while ((half + 1) * (half + 1) <= rem) ++half;
                    if (half == h) t.push_back(((dz + r) << 16) | (dy + r));
                }
        }
        t[r + 1] = (int)t.size() - (r + 2);
        hipError_t st = hipMalloc(&S->tab_dev[r], t.size() * sizeof(int));
        if (st != hipSuccess) { S->tab_dev[r] = nullptr; return st; }
        st = hipMemcpyAsync(S->tab_dev[r], t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice, s);   // tab_host outlives the copy
        if (st != hipSuccess) return st;
    }
    *out = S->tab_dev[r];
    return hipSuccess;
}

// one dilation (erode = false) or erosion of a packed (Z,H,W) volume
hipError_t mo_ball(MoState* S, const uint32_t* in, uint32_t* out, int Z, int H, int W, int r, bool erode, hipStream_t s) {
    const int* tab = nullptr;
    hipError_t st = mo_ball_table(S, r, s, &tab);
    if (st != hipSuccess) return st;
    const int WW = (W + 31) / 32;
    const int TW = WW > 4 ? 8 : (WW > 2 ? 4 : 2), TY = 256 / TW;
    const size_t lds = (size_t)(2 * r + 1) * (TY + 2 * r) * (TW + 2) * sizeof(uint32_t);       // <= 33 * 160 * 4 * 4 = 84 480 bytes
    const dim3 grid((WW + TW - 1) / TW, (H + TY - 1) / TY, (Z + MO_ZC - 1) / MO_ZC);
    if (erode) hipLaunchKernelGGL(mo_ball_kernel<true>, grid, dim3(256), lds, s, in, out, Z, H, WW, W, r, TW, tab);
    else hipLaunchKernelGGL(mo_ball_kernel<false>, grid, dim3(256), lds, s, in, out, Z, H, WW, W, r, TW, tab);
    return hipGetLastError();
}

hipError_t mo_ball_attrs() {                                   // per device and cheap: set on every call, as smooth3d.hip does
    hipError_t st = hipFuncSetAttribute((const void*)mo_ball_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, MO_LDS_LIMIT);
    if (st == hipSuccess) st = hipFuncSetAttribute((const void*)mo_ball_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, MO_LDS_LIMIT);
    return st;
}

struct CcWs { uint32_t *lab = nullptr, *sizes = nullptr, *ov = nullptr; unsigned long long* best = nullptr; };

// mode 0: out = m where the component has >= min_size voxels (and passes the surface test against `org` when given);
// mode 1: out = m on the largest component.  kept_voxels / comps: optional device counters (added to).  No synchronisation.
hipError_t cc6_run(const CcWs& w, const uint8_t* m, int Z, int H, int W, int mode, uint32_t min_size, const uint8_t* org, uint8_t* out,
                   uint32_t* kept_voxels, uint32_t* comps, hipStream_t s) {
    const int64_t n = (int64_t)Z * H * W, rows = (int64_t)Z * H;
    const unsigned vox_blocks = eng_blocks(n);
    uint32_t* ov = (mode == 0 && org) ? w.ov : nullptr;
    ccl_init(m, w.lab, w.sizes, ov, W, rows, s);
    hipLaunchKernelGGL(cc6_merge_kernel, dim3(vox_blocks), dim3(256), 0, s, m, w.lab, Z, H, W);
    ccl_flatten(w.lab, n, vox_blocks, s);
    ccl_count(w.lab, w.sizes, W, rows, s);
    if (mode == 0) {
        if (ov) hipLaunchKernelGGL(cc6_overlap_kernel, dim3(vox_blocks), dim3(256), 0, s, (const uint32_t*)w.lab, org, ov, Z, H, W);
        hipLaunchKernelGGL(cc6_filter_kernel, dim3(vox_blocks), dim3(256), 0, s, m, (const uint32_t*)w.lab, (const uint32_t*)w.sizes, (const uint32_t*)ov,
                           min_size, out, n, kept_voxels, comps);
    } else {
        hipError_t st = hipMemsetAsync(w.best, 0, 8, s);
        if (st != hipSuccess) return st;
        hipLaunchKernelGGL(cc6_best_kernel, dim3(vox_blocks), dim3(256), 0, s, (const uint32_t*)w.lab, (const uint32_t*)w.sizes, n, w.best, comps);
        hipLaunchKernelGGL(cc6_largest_kernel, dim3(vox_blocks), dim3(256), 0, s, m, (const uint32_t*)w.lab, (const unsigned long long*)w.best, out, n);
    }
    return hipGetLastError();
}

template <typename T, bool LABEL>
void mo_pack(const T* src, int64_t sz, int64_t sy, uint32_t label, const uint8_t* zflag, int dz, int dy, int dx, uint32_t* out, hipStream_t s) {
    const int64_t rows = (int64_t)dz * dy, pieces = rows * ((dx + 63) / 64);
    hipLaunchKernelGGL((mo_pack_kernel<T, LABEL>), dim3((unsigned)((pieces + 3) / 4)), dim3(256), 0, s, src, sz, sy, label, zflag, dy, rows, dx,
                       (dx + 31) / 32, out);
}
inline void mo_pack_bytes(const uint8_t* src, int dz, int dy, int dx, uint32_t* out, hipStream_t s) {
    mo_pack<uint8_t, false>(src, (int64_t)dy * dx, dx, 0u, nullptr, dz, dy, dx, out, s);
}
inline void mo_unpack(const uint32_t* a, const uint32_t* b, const uint32_t* alt, const uint32_t* counter, int dz, int dy, int dx, uint8_t* out,
                      hipStream_t s) {
    const int64_t rows = (int64_t)dz * dy;
    hipLaunchKernelGGL(mo_unpack_kernel, dim3(eng_blocks(rows * dx)), dim3(256), 0, s, a, b, alt, counter, rows, dx, (dx + 31) / 32, out);
}
}  // namespace

void refine_release(saber_engine* e) {
    MoState* S = (MoState*)e->refine_state;
    if (!S) return;
    for (int* p : S->tab_dev) (void)hipFree(p);
    (void)hipFree(S->bits);
    delete S;
    e->refine_state = nullptr;
}

extern "C" int saber_morph_ball_3d(saber_engine* e, const uint8_t* mask_dev, int Z, int H, int W, int radius, int op, uint8_t* out_dev,
                                   void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!mask_dev || !out_dev || Z <= 0 || H <= 0 || W <= 0) return eng_fail(e, SABER_ERR_INVALID, "morph_ball_3d: bad argument");
    if (radius < 1 || radius > MO_MAX_R) return eng_fail(e, SABER_ERR_INVALID, "morph_ball_3d: radius must lie in 1..16");
    if (op < 0 || op > 2) return eng_fail(e, SABER_ERR_INVALID, "morph_ball_3d: op must be 0 (dilate), 1 (erode) or 2 (open)");
    if ((int64_t)Z * H * W >= (int64_t)0x7fffffff) return eng_fail(e, SABER_ERR_INVALID, "morph_ball_3d: volumes of 2^31 voxels or more are not supported");
    hipStream_t s = (hipStream_t)stream;
    uint32_t *pa = nullptr, *pb = nullptr;
    auto cleanup = [&]() { (void)hipFree(pa); (void)hipFree(pb); };
    ENG_DEVICE(e);
    MoState* S = mo_state(e);
    const size_t words = (size_t)Z * H * ((W + 31) / 32);
    ENG_HIP_CLEANUP(e, mo_ball_attrs());
    ENG_HIP_CLEANUP(e, hipMalloc(&pa, words * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&pb, words * 4));
    mo_pack_bytes(mask_dev, Z, H, W, pa, s);
    ENG_HIP_CLEANUP(e, mo_ball(S, pa, pb, Z, H, W, radius, op != 0, s));
    if (op == 2) ENG_HIP_CLEANUP(e, mo_ball(S, pb, pa, Z, H, W, radius, false, s));
    mo_unpack(op == 2 ? pa : pb, nullptr, nullptr, nullptr, Z, H, W, out_dev, s);
    ENG_HIP_CLEANUP(e, hipGetLastError());
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
    cleanup();
    return SABER_OK;
}

extern "C" int saber_components6_3d(saber_engine* e, const uint8_t* mask_dev, int Z, int H, int W, int mode, int min_size, uint8_t* out_dev,
                                    int* out_n_components, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!mask_dev || !out_dev || Z <= 0 || H <= 0 || W <= 0) return eng_fail(e, SABER_ERR_INVALID, "components6_3d: bad argument");
    if (mode != 0 && mode != 1) return eng_fail(e, SABER_ERR_INVALID, "components6_3d: mode must be 0 (drop below min_size) or 1 (keep the largest)");
    const int64_t n = (int64_t)Z * H * W;
    if (n >= (int64_t)0x7fffffff) return eng_fail(e, SABER_ERR_INVALID, "components6_3d: volumes of 2^31 voxels or more are not supported");
    hipStream_t s = (hipStream_t)stream;
    CcWs w;
    uint32_t* counter = nullptr;
    auto cleanup = [&]() { (void)hipFree(w.lab); (void)hipFree(w.sizes); (void)hipFree(w.best); (void)hipFree(counter); };
    ENG_DEVICE(e);
    if (out_n_components) *out_n_components = 0;
    ENG_HIP_CLEANUP(e, hipMalloc(&w.lab, (size_t)n * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&w.sizes, (size_t)n * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&w.best, 8));
    ENG_HIP_CLEANUP(e, hipMalloc(&counter, 4));
    ENG_HIP_CLEANUP(e, hipMemsetAsync(counter, 0, 4, s));
    ENG_HIP_CLEANUP(e, cc6_run(w, mask_dev, Z, H, W, mode, (uint32_t)std::max(min_size, 0), nullptr, out_dev, nullptr, counter, s));
    uint32_t k = 0;
    ENG_HIP_CLEANUP(e, hipMemcpyAsync(&k, counter, 4, hipMemcpyDeviceToHost, s));
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
    cleanup();
    if (out_n_components) *out_n_components = (int)k;        // mode 0: components kept; mode 1: components found
    return SABER_OK;
}

namespace {
struct RfScratch {
    uint8_t *trim = nullptr, *clean = nullptr, *zflag = nullptr, *b_org = nullptr, *b_cl = nullptr, *b_comb = nullptr, *b_t = nullptr;
    uint32_t *flags = nullptr, *p_org = nullptr, *p_mem = nullptr, *p_a = nullptr, *p_b = nullptr, *p_c = nullptr;
    CcWs cc;
    void release() {
        (void)hipFree(trim); (void)hipFree(clean); (void)hipFree(zflag); (void)hipFree(b_org); (void)hipFree(b_cl); (void)hipFree(b_comb); (void)hipFree(b_t);
        (void)hipFree(flags); (void)hipFree(p_org); (void)hipFree(p_mem); (void)hipFree(p_a); (void)hipFree(p_b);
        (void)hipFree(p_c); (void)hipFree(cc.lab); (void)hipFree(cc.sizes); (void)hipFree(cc.ov); (void)hipFree(cc.best);
    }
};

struct RfCand { MoPair p; int dilate_r, open_r; };

template <typename T>
int refine_run(saber_engine* e, const T* org, const uint8_t* mem, int Z, int H, int W, const saber_refine_params* P, T* org_out, T* mem_out,
               int* out_n_labels_in, int* out_n_pairs, hipStream_t s) {
    const int64_t n = (int64_t)Z * H * W, plane = (int64_t)H * W;
    RfScratch R;
    auto cleanup = [&]() { R.release(); };
    ENG_DEVICE(e);
    MoState* S = mo_state(e);
    // the pairs of the previous call go now
    S->pairs.clear();
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));
    (void)hipFree(S->bits);
    S->bits = nullptr;
    S->Z = Z; S->H = H; S->W = W;
    ENG_HIP_CLEANUP(e, mo_ball_attrs());
    ENG_HIP_CLEANUP(e, hipMemsetAsync(org_out, 0, (size_t)n * sizeof(T), s));
    ENG_HIP_CLEANUP(e, hipMemsetAsync(mem_out, 0, (size_t)n * sizeof(T), s));
    // ---- step 1 (run, :466-471): trim the membrane, drop its 6-connected components below min_membrane_area
    ENG_HIP_CLEANUP(e, hipMalloc(&R.trim, (size_t)n));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.clean, (size_t)n));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.zflag, (size_t)Z));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.cc.lab, (size_t)n * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.cc.sizes, (size_t)n * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.cc.best, 8));
    const int tz = P->edge_trim_z, txy = P->edge_trim_xy;
    int z0 = 0, z1 = 0, y0 = 0, y1 = 0, x0 = 0, x1 = 0;        // empty boxes unless the trims are usable
    if (tz > 0 && tz < Z / 2) { z0 = tz; z1 = Z - tz; }
    if (txy > 0 && txy < H / 2 && txy < W / 2) { y0 = txy; y1 = H - txy; x0 = txy; x1 = W - txy; }
    hipLaunchKernelGGL(mo_trim_kernel, dim3(eng_blocks(n)), dim3(256), 0, s, mem, R.trim, Z, H, W, z0, z1, y0, y1, x0, x1);
    ENG_HIP_CLEANUP(e, cc6_run(R.cc, R.trim, Z, H, W, 0, (uint32_t)std::max(P->min_membrane_area, 0), nullptr, R.clean, nullptr, nullptr, s));
    // ---- step 2 (:473-476): organelles only count on planes that hold membrane
    ENG_HIP_CLEANUP(e, hipMemsetAsync(R.zflag, 0, (size_t)Z, s));
    hipLaunchKernelGGL(mo_zpresence_kernel, dim3((unsigned)std::min<int64_t>((plane + 255) / 256, 64), Z), dim3(256), 0, s, (const uint8_t*)R.clean, plane,
                       R.zflag);
    // ---- step 3 (:478-480): the labels present, with voxel count and bounding box
    const void* org_buf = org;
    uint32_t maxv = 0;
    ENG_HIP_CLEANUP(e, label_max_host(&org_buf, &n, 1, sizeof(T), R.zflag, plane, &maxv, s));      // synchronisation 1
    if (maxv == 0) { cleanup(); return SABER_OK; }
    if (maxv > MO_MAX_LABEL) { cleanup(); return eng_fail(e, SABER_ERR_INVALID, "refine_membranes: label values above 2^22 are not supported"); }
    const uint64_t type_max = sizeof(T) == 1 ? 0xffull : (sizeof(T) == 2 ? 0xffffull : 0xffffffffull);
    if (((uint64_t)maxv + 1) * 2 > type_max) {
        cleanup();
        return eng_fail(e, SABER_ERR_INVALID, "refine_membranes: (largest label + 1) * 2 = " + std::to_string(((uint64_t)maxv + 1) * 2) +
                                                  " does not fit the label type (the reference would wrap silently)");
    }
    const size_t n_stats = (size_t)maxv + 1;
    std::vector<uint32_t> st;
    ENG_HIP_CLEANUP(e, label_stats_host(&org_buf, &Z, 1, sizeof(T), R.zflag, H, W, n_stats, st, s));      // synchronisation 2
    // ---- host: ROI per label (_get_organelle_roi, :251-272) and the shape-dependent radii (:364-374)
    std::vector<RfCand> cands;
    const int pad = P->ball_size / 2;
    const int dims[3] = {Z, H, W};
    int n_in = 0;
    int64_t roi_max = 0;
    size_t bit_words = 0, roi_words_max = 0;
    for (size_t v = 1; v < n_stats; ++v) {
        const uint32_t* p = &st[v * 8];
        if (!p[0]) continue;
        ++n_in;
        int lo[3], hi[3];
        bool small = false;
        for (int a = 0; a < 3; ++a) {
            lo[a] = (int)p[1 + a]; hi[a] = (int)p[4 + a] + 1;
            if ((float)(hi[a] - lo[a]) < P->min_roi_size[a]) small = true;     // the reference's float32 comparison (:261-266)
        }
        if (small) continue;
        for (int a = 0; a < 3; ++a) { lo[a] = std::max(lo[a] - pad, 0); hi[a] = std::min(hi[a] + pad, dims[a]); }
        RfCand c;
        c.p.label = (uint32_t)v;
        c.p.z0 = lo[0]; c.p.y0 = lo[1]; c.p.x0 = lo[2];
        c.p.dz = hi[0] - lo[0]; c.p.dy = hi[1] - lo[1]; c.p.dx = hi[2] - lo[2];
        const int mx = std::max(c.p.dz, std::max(c.p.dy, c.p.dx)), mn = std::min(c.p.dz, std::min(c.p.dy, c.p.dx));
        const bool elongated = mx > 3 * mn;                     // float32 max / min > 3.0 on integer extents
        c.dilate_r = elongated ? 1 : 2;
        c.open_r = elongated ? std::max(1, P->ball_size / 2) : P->ball_size;
        const size_t words = (size_t)c.p.dz * c.p.dy * ((c.p.dx + 31) / 32);
        c.p.off_org = bit_words; c.p.off_mem = bit_words + words;
        bit_words += 2 * words;
        roi_words_max = std::max(roi_words_max, words);
        roi_max = std::max(roi_max, (int64_t)c.p.dz * c.p.dy * c.p.dx);
        cands.push_back(c);
    }
    if (out_n_labels_in) *out_n_labels_in = n_in;
    if (cands.empty()) { ENG_HIP_CLEANUP(e, hipStreamSynchronize(s)); cleanup(); return SABER_OK; }
    ENG_HIP_CLEANUP(e, hipMalloc(&S->bits, bit_words * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.flags, cands.size() * 8));
    ENG_HIP_CLEANUP(e, hipMemsetAsync(R.flags, 0, cands.size() * 8, s));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.b_org, (size_t)roi_max));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.b_cl, (size_t)roi_max));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.b_comb, (size_t)roi_max));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.b_t, (size_t)roi_max));
    if (P->keep_surface_membranes) ENG_HIP_CLEANUP(e, hipMalloc(&R.cc.ov, (size_t)roi_max * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.p_org, roi_words_max * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.p_mem, roi_words_max * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.p_a, roi_words_max * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.p_b, roi_words_max * 4));
    ENG_HIP_CLEANUP(e, hipMalloc(&R.p_c, roi_words_max * 4));
    // ---- per organelle, ascending label (_process_organelle_batch, :335-443); nothing below waits for the device
    for (size_t i = 0; i < cands.size(); ++i) {
        const RfCand& c = cands[i];
        const int dz = c.p.dz, dy = c.p.dy, dx = c.p.dx;
        const int64_t rn = (int64_t)dz * dy * dx, words = (int64_t)dz * dy * ((dx + 31) / 32);
        const int64_t origin = ((int64_t)c.p.z0 * H + c.p.y0) * W + c.p.x0;
        uint32_t* kept = R.flags + 2 * i;                       // voxels of the cleaned membrane: 0 = the organelle is dropped (:384, :399)
        uint32_t* opened = R.flags + 2 * i + 1;                 // voxels the opening left: 0 = fall back to the unopened mask (:414-416)
        const unsigned vb = eng_blocks(rn);
        mo_pack<T, true>(org + origin, plane, W, c.p.label, R.zflag + c.p.z0, dz, dy, dx, R.p_org, s);
        mo_pack<uint8_t, false>(R.clean + origin, plane, W, 0u, nullptr, dz, dy, dx, R.p_mem, s);
        // enhanced membrane = dilate(membrane) AND dilate(organelle)   (:376-382)
        ENG_HIP_CLEANUP(e, mo_ball(S, R.p_mem, R.p_a, dz, dy, dx, c.dilate_r, false, s));
        ENG_HIP_CLEANUP(e, mo_ball(S, R.p_org, R.p_b, dz, dy, dx, c.dilate_r, false, s));
        mo_unpack(R.p_a, R.p_b, nullptr, nullptr, dz, dy, dx, R.b_t, s);
        mo_unpack(R.p_org, nullptr, nullptr, nullptr, dz, dy, dx, R.b_org, s);
        // components >= 100 voxels (:393), on the organelle's surface when asked (:396-397)
        ENG_HIP_CLEANUP(e, cc6_run(R.cc, R.b_t, dz, dy, dx, 0, 100u, P->keep_surface_membranes ? R.b_org : nullptr, R.b_cl, kept, nullptr, s));
        // combined = (organelle - membrane) != 0: the organelle's value is >= 4, so this is organelle OR membrane (:403-408)
        hipLaunchKernelGGL(mo_bytes_op_kernel, dim3(vb), dim3(256), 0, s, (const uint8_t*)R.b_org, (const uint8_t*)R.b_cl, 0, R.b_comb, rn);
        mo_pack_bytes(R.b_comb, dz, dy, dx, R.p_a, s);
        // opening (:410-420), then its largest component (:423)
        ENG_HIP_CLEANUP(e, mo_ball(S, R.p_a, R.p_b, dz, dy, dx, c.open_r, true, s));
        ENG_HIP_CLEANUP(e, mo_ball(S, R.p_b, R.p_c, dz, dy, dx, c.open_r, false, s));
        hipLaunchKernelGGL(mo_popcount_kernel, dim3(eng_blocks(words)), dim3(256), 0, s, (const uint32_t*)R.p_c, words, opened);
        mo_unpack(R.p_c, nullptr, R.p_a, opened, dz, dy, dx, R.b_comb, s);
        ENG_HIP_CLEANUP(e, cc6_run(R.cc, R.b_comb, dz, dy, dx, 1, 0u, nullptr, R.b_comb, nullptr, nullptr, s));
        // organelle AND combined -> largest component (:426-427); membrane AND combined -> components >= 50 voxels (:430-431)
        hipLaunchKernelGGL(mo_bytes_op_kernel, dim3(vb), dim3(256), 0, s, (const uint8_t*)R.b_org, (const uint8_t*)R.b_comb, 1, R.b_t, rn);
        ENG_HIP_CLEANUP(e, cc6_run(R.cc, R.b_t, dz, dy, dx, 1, 0u, nullptr, R.b_t, nullptr, nullptr, s));
        hipLaunchKernelGGL(mo_bytes_op_kernel, dim3(vb), dim3(256), 0, s, (const uint8_t*)R.b_cl, (const uint8_t*)R.b_comb, 1, R.b_cl, rn);
        ENG_HIP_CLEANUP(e, cc6_run(R.cc, R.b_cl, dz, dy, dx, 0, 50u, nullptr, R.b_cl, nullptr, nullptr, s));
        // keep the pair compactly, write it into the label maps: organelle v comes out as v + 1 (:494-495, :437, :539-540)
        mo_pack_bytes(R.b_t, dz, dy, dx, S->bits + c.p.off_org, s);
        mo_pack_bytes(R.b_cl, dz, dy, dx, S->bits + c.p.off_mem, s);
        hipLaunchKernelGGL(mo_scatter_kernel<T>, dim3(vb), dim3(256), 0, s, (const uint8_t*)R.b_t, (const uint8_t*)R.b_cl, (const uint32_t*)kept,
                           (T)(c.p.label + 1), dz, dy, dx, H, W, c.p.z0, c.p.y0, c.p.x0, org_out, mem_out);
        ENG_HIP_CLEANUP(e, hipGetLastError());
    }
    std::vector<uint32_t> flags(cands.size() * 2);
    ENG_HIP_CLEANUP(e, hipMemcpyAsync(flags.data(), R.flags, flags.size() * 4, hipMemcpyDeviceToHost, s));
    ENG_HIP_CLEANUP(e, hipStreamSynchronize(s));                        // synchronisation 3
    for (size_t i = 0; i < cands.size(); ++i)
        if (flags[2 * i]) S->pairs.push_back(cands[i].p);
    if (out_n_pairs) *out_n_pairs = (int)S->pairs.size();
    cleanup();
    return SABER_OK;
}
}  // namespace

extern "C" int saber_refine_membranes(saber_engine* e, const void* org_dev, int elem_bytes, const uint8_t* mem_dev, int Z, int H, int W,
                                      const saber_refine_params* params, void* org_labels_out_dev, void* mem_labels_out_dev, int* out_n_labels_in,
                                      int* out_n_pairs, void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (!org_dev || !mem_dev || !params || !org_labels_out_dev || !mem_labels_out_dev || Z <= 0 || H <= 0 || W <= 0)
        return eng_fail(e, SABER_ERR_INVALID, "refine_membranes: bad argument");
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return eng_fail(e, SABER_ERR_INVALID, "refine_membranes: elem_bytes must be 1, 2 or 4");
    if (params->ball_size < 1 || params->ball_size > MO_MAX_R) return eng_fail(e, SABER_ERR_INVALID, "refine_membranes: ball_size (a radius) must lie in 1..16");
    if (params->edge_trim_z < 0 || params->edge_trim_xy < 0) return eng_fail(e, SABER_ERR_INVALID, "refine_membranes: negative edge trim");
    if ((int64_t)Z * H * W >= (int64_t)0x7fffffff) return eng_fail(e, SABER_ERR_INVALID, "refine_membranes: volumes of 2^31 voxels or more are not supported");
    if (out_n_labels_in) *out_n_labels_in = 0;
    if (out_n_pairs) *out_n_pairs = 0;
    hipStream_t s = (hipStream_t)stream;
    if (elem_bytes == 1)
        return refine_run(e, (const uint8_t*)org_dev, mem_dev, Z, H, W, params, (uint8_t*)org_labels_out_dev, (uint8_t*)mem_labels_out_dev, out_n_labels_in, out_n_pairs, s);
    if (elem_bytes == 2)
        return refine_run(e, (const uint16_t*)org_dev, mem_dev, Z, H, W, params, (uint16_t*)org_labels_out_dev, (uint16_t*)mem_labels_out_dev, out_n_labels_in, out_n_pairs, s);
    return refine_run(e, (const uint32_t*)org_dev, mem_dev, Z, H, W, params, (uint32_t*)org_labels_out_dev, (uint32_t*)mem_labels_out_dev, out_n_labels_in, out_n_pairs, s);
}

template <typename T>
static void mo_expand_pairs(const MoState* S, int first, int count, T* org_stack, T* mem_stack, hipStream_t s) {
    const int64_t n = (int64_t)S->Z * S->H * S->W;
    for (int k = 0; k < count; ++k) {
        const MoPair& p = S->pairs[first + k];
        const int WW = (p.dx + 31) / 32;
        const unsigned vb = eng_blocks((int64_t)p.dz * p.dy * p.dx);
        hipLaunchKernelGGL(mo_expand_kernel<T>, dim3(vb), dim3(256), 0, s, (const uint32_t*)(S->bits + p.off_org), (T)(p.label + 1), p.dz, p.dy, p.dx, WW,
                           S->H, S->W, p.z0, p.y0, p.x0, org_stack + (int64_t)k * n);
        hipLaunchKernelGGL(mo_expand_kernel<T>, dim3(vb), dim3(256), 0, s, (const uint32_t*)(S->bits + p.off_mem), (T)(p.label + 1), p.dz, p.dy, p.dx, WW,
                           S->H, S->W, p.z0, p.y0, p.x0, mem_stack + (int64_t)k * n);
    }
}

extern "C" int saber_refine_membranes_instances(saber_engine* e, int first, int count, int elem_bytes, void* org_stack_dev, void* mem_stack_dev,
                                                void* stream) {
    if (!e) return SABER_ERR_INVALID;
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return eng_fail(e, SABER_ERR_INVALID, "refine_membranes_instances: elem_bytes must be 1, 2 or 4");
    MoState* S = (MoState*)e->refine_state;
    const int n_pairs = S ? (int)S->pairs.size() : 0;
    if (first < 0 || count < 0 || first > n_pairs || count > n_pairs - first)
        return eng_fail(e, SABER_ERR_INVALID, "refine_membranes_instances: pairs [" + std::to_string(first) + ", " + std::to_string((int64_t)first + count) +
                                                  ") lie outside [0, " + std::to_string(n_pairs) + ")");
    if (count == 0) return SABER_OK;
    if (!org_stack_dev || !mem_stack_dev) return eng_fail(e, SABER_ERR_INVALID, "refine_membranes_instances: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ENG_DEVICE(e);
    const size_t bytes = (size_t)count * S->Z * S->H * S->W * elem_bytes;
    ENG_HIP(e, hipMemsetAsync(org_stack_dev, 0, bytes, s));
    ENG_HIP(e, hipMemsetAsync(mem_stack_dev, 0, bytes, s));
    if (elem_bytes == 1) mo_expand_pairs(S, first, count, (uint8_t*)org_stack_dev, (uint8_t*)mem_stack_dev, s);
    else if (elem_bytes == 2) mo_expand_pairs(S, first, count, (uint16_t*)org_stack_dev, (uint16_t*)mem_stack_dev, s);
    else mo_expand_pairs(S, first, count, (uint32_t*)org_stack_dev, (uint32_t*)mem_stack_dev, s);
    ENG_HIP(e, hipGetLastError());
    return SABER_OK;
}
