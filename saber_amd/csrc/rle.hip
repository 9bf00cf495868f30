// Run-length form of the mask generator's masks on the device: upstream's uncompressed RLE (sam2 utils/amg.py: mask_to_rle_pytorch /
// rle_to_mask; SAM2AutomaticMaskGenerator(output_mode="uncompressed_rle")).  A mask is flattened in COLUMN-major order, pixel (y, x) has
// position p = x H + y; `counts` alternates runs of zeros and ones and starts with a zeros run (0 when pixel (0,0) is set); the entries sum
// to H W.  Input of the encoder and output of the decoder are the generator's bit-packed rows: (n, H, W32) uint32, bit b of word w of a row =
// pixel 32w+b; bits at x >= W are ignored on input and zero on output.
//
// With t(p) = bit(p) ^ bit(p - 1), bit(-1) = 0, a mask with T transitions t_0 < ... < t_{T-1} has T + 1 entries:
//   counts[k] = t_k - t_{k-1},  t_{-1} = 0,  t_T = H W.
// Encoder, one wave per (mask, word column w), a lane per row, 64 rows per step:
//   rle_colcount   the XOR of a row's word with the word of the row above gives the transitions of 32 columns at once (row 0 compares with
//                  row H-1 of the column before: the last row's word shifted by one, bit 31 of word w-1 carried in); per column one ballot
//                  = the transitions of 64 rows in column-major order.  Per (mask, column): their number and the position of the last one
//   rle_colscan    a block per mask: exclusive sum of the numbers (the rank of a column's first transition) and exclusive maximum of the
//                  last positions (the transition before the column's first one), in place; the mask's T
//   rle_offsets    one block: exclusive sum of T + 1 over the masks, 64-bit -> offsets[n + 1]
//   rle_write      the walk of rle_colcount again: a transition of rank k at p writes counts[offset + k] = p - (the transition before it: the
//                  next lower bit of the ballot, the column's carry, or the scan's value); the wave of the last word column writes the
//                  closing entry H W - t_{T-1}
// Only the columns with a transition in the step's 64 rows are balloted (rle_active_columns).
// No atomics: every entry has one writer and its value does not depend on the order anything ran in.
// Decoder: bits_out <- 0; rle_toggle, a block per mask, sums the counts (clamped at H W) and flips, per run of ones, the pixel where it
// starts and the pixel behind its end (flips at one place cancel: empty runs), plus pixel (0, 32w) of every word column w >= 1 the run
// enters from the column before - so a word column no longer depends on the ones before it; rle_sweep, a wave per (mask, word column),
// turns the flips into values: the parity of the flips above in the column, started with the parity of the word's columns before it.
#include <algorithm>
#include <cstdio>

#include "kernels.h"

namespace {

constexpr int RLE_WAVES = 4;                       // waves of a block of the per-word-column kernels
constexpr int64_t RLE_MAX_BLOCKS = 1 << 20;        // the (mask, word column) pairs beyond that many blocks are walked in a grid-stride loop

inline size_t rle_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct RleWs {
    uint32_t* rank;      // [n W]  rle_colcount: transitions of the column; rle_colscan: transitions of the mask's columns before it
    uint32_t* prev;      // [n W]  rle_colcount: position of the column's last transition (0: none); rle_colscan: of the last one before the column
    uint32_t* total;     // [n]    T of the mask
};

inline RleWs rle_carve(void* ws, int n, int W) {
    RleWs r;
    const size_t cols = rle_align((size_t)n * (size_t)W * 4);
    r.rank = (uint32_t*)ws;
    r.prev = (uint32_t*)((char*)ws + cols);
    r.total = (uint32_t*)((char*)ws + 2 * cols);
    return r;
}

}  // namespace

// The transitions of rows y0 .. y0+63 of word column w of one mask: bit c of the result of lane l = pixel (y0 + l, 32 w + c) differs from the
// pixel before it in column-major order.  `above0`: what row 0 compares with; `carry`: the word of row y0 - 1 (in, y0 > 0) / y0 + 63 (out).
__device__ __forceinline__ uint32_t rle_transitions(const uint32_t* __restrict__ col, int W32, int H, int y0, int lane, uint32_t above0, uint32_t& carry) {
    const int y = y0 + lane;
    const bool in = y < H;
    const uint32_t word = in ? col[(int64_t)y * W32] : 0u;
    uint32_t above = __shfl_up(word, 1, 64);
    if (lane == 0) above = y0 == 0 ? above0 : carry;
    carry = __shfl(word, 63, 64);
    return in ? word ^ above : 0u;
}

// The columns of the word (bits of `valid`) with a transition in the wave's 64 rows, the same value in every lane.  Masks are blobs: most
// steps have none, and the per-column ballots are spent on those that have.
__device__ __forceinline__ uint32_t rle_active_columns(uint32_t t, uint32_t valid) {
    t &= valid;
    if (__ballot(t != 0u) == 0ull) return 0u;                      // wave-uniform
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) t |= __shfl_xor(t, d, 64);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
}

// what row 0 of word column w compares with: row H-1, one column to the left
__device__ __forceinline__ uint32_t rle_above0(const uint32_t* __restrict__ mask, int W32, int H, int w) {
    const uint32_t* last = mask + (int64_t)(H - 1) * W32;
    return (last[w] << 1) | (w > 0 ? last[w - 1] >> 31 : 0u);
}

__global__ __launch_bounds__(64 * RLE_WAVES) void rle_colcount_kernel(const uint32_t* __restrict__ bits, int H, int W, int W32, int64_t pairs,
                                                                      uint32_t* __restrict__ cnt, uint32_t* __restrict__ last) {
    const int lane = threadIdx.x & 63;
    for (int64_t pair = (int64_t)blockIdx.x * RLE_WAVES + (threadIdx.x >> 6); pair < pairs; pair += (int64_t)gridDim.x * RLE_WAVES) {      // wave-uniform
        const int64_t m = pair / W32;
        const int w = (int)(pair - m * W32);
        const int ncols = min(32, W - 32 * w);
        const uint32_t valid = ncols == 32 ? 0xffffffffu : (1u << ncols) - 1u;      // bits at x >= W are not pixels
        const uint32_t* mask = bits + m * H * W32;
        const uint32_t above0 = rle_above0(mask, W32, H, w);
        uint32_t carry = 0u, my_cnt = 0u, my_last = 0u;            // lane c: column 32 w + c
        for (int y0 = 0; y0 < H; y0 += 64) {
            const uint32_t t = rle_transitions(mask + w, W32, H, y0, lane, above0, carry);
            uint32_t cols = rle_active_columns(t, valid);
            while (cols) {                                         // wave-uniform
                const int c = __builtin_ctz(cols);
                cols &= cols - 1u;
                const unsigned long long b = __ballot((t >> c) & 1u);
                if (lane == c) {
                    my_cnt += (uint32_t)__popcll(b);
                    my_last = (uint32_t)(32 * w + c) * (uint32_t)H + (uint32_t)(y0 + 63 - __clzll((long long)b));
                }
            }
        }
        if (lane < ncols) {
            const int64_t i = m * W + 32 * w + lane;
            cnt[i] = my_cnt;
            last[i] = my_last;
        }
    }
}

// block-wide inclusive (sum, max) over 256 threads; returns the inclusive values and the block's totals
__device__ __forceinline__ void rle_block_scan(uint32_t& s, uint32_t& mx, uint32_t& tot_s, uint32_t& tot_mx, uint32_t (*sh)[2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t os = __shfl_up(s, d, 64), om = __shfl_up(mx, d, 64);
        if (lane >= d) {
            s += os;
            mx = max(mx, om);
        }
    }
    __syncthreads();                                               // the last round's readers are done with sh
    if (lane == 63) {
        sh[wave][0] = s;
        sh[wave][1] = mx;
    }
    __syncthreads();
    tot_s = 0u;
    tot_mx = 0u;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        if (v == wave) {
            s += tot_s;
            mx = max(mx, tot_mx);
        }
        tot_s += sh[v][0];
        tot_mx = max(tot_mx, sh[v][1]);
    }
}

__global__ __launch_bounds__(256) void rle_colscan_kernel(uint32_t* __restrict__ rank, uint32_t* __restrict__ prev, uint32_t* __restrict__ total, int W) {
    __shared__ uint32_t sh[4][2];
    uint32_t* r = rank + (int64_t)blockIdx.x * W;
    uint32_t* p = prev + (int64_t)blockIdx.x * W;
    uint32_t run_s = 0u, run_mx = 0u;
    for (int64_t x0 = 0; x0 < W; x0 += 256) {                      // block-uniform
        const int64_t x = x0 + (int64_t)threadIdx.x;
        const uint32_t c = x < W ? r[x] : 0u, l = x < W ? p[x] : 0u;
        uint32_t s = c, mx = l, tot_s, tot_mx;
        rle_block_scan(s, mx, tot_s, tot_mx, sh);
        // exclusive: the sum without the column's own number; the maximum of the columns before = the inclusive one of the neighbour
        uint32_t ex_mx = __shfl_up(mx, 1, 64);
        if ((threadIdx.x & 63) == 0) ex_mx = 0u;
        __syncthreads();
        if ((threadIdx.x & 63) == 63) sh[threadIdx.x >> 6][1] = mx;
        __syncthreads();
        if ((threadIdx.x & 63) == 0 && threadIdx.x > 0) ex_mx = sh[(threadIdx.x >> 6) - 1][1];
        if (x < W) {
            r[x] = run_s + s - c;
            p[x] = max(run_mx, ex_mx);
        }
        run_s += tot_s;
        run_mx = max(run_mx, tot_mx);
    }
    if (threadIdx.x == 0) total[blockIdx.x] = run_s;
}

__global__ __launch_bounds__(256) void rle_offsets_kernel(const uint32_t* __restrict__ total, int n, int64_t* __restrict__ offsets) {
    __shared__ int64_t sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t run = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {                          // block-uniform
        const int i = i0 + (int)threadIdx.x;
        const int64_t v = i < n ? (int64_t)total[i] + 1 : 0;
        int64_t s = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(s, d, 64);
            if (lane >= d) s += o;
        }
        __syncthreads();
        if (lane == 63) sh[wave] = s;
        __syncthreads();
        int64_t tot = 0;
#pragma unroll
        for (int v4 = 0; v4 < 4; ++v4) {
            if (v4 == wave) s += tot;
            tot += sh[v4];
        }
        if (i < n) offsets[i] = run + s - v;
        run += tot;
    }
    if (threadIdx.x == 0) offsets[n] = run;
}

__global__ __launch_bounds__(64 * RLE_WAVES) void rle_write_kernel(const uint32_t* __restrict__ bits, int H, int W, int W32, int64_t pairs,
                                                                   const uint32_t* __restrict__ rank, const uint32_t* __restrict__ prev,
                                                                   const int64_t* __restrict__ offsets, uint32_t* __restrict__ counts, int64_t capacity) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below_me = (1ull << lane) - 1ull;
    for (int64_t pair = (int64_t)blockIdx.x * RLE_WAVES + (threadIdx.x >> 6); pair < pairs; pair += (int64_t)gridDim.x * RLE_WAVES) {      // wave-uniform
        const int64_t m = pair / W32;
        const int w = (int)(pair - m * W32);
        const int ncols = min(32, W - 32 * w);
        const uint32_t valid = ncols == 32 ? 0xffffffffu : (1u << ncols) - 1u;      // bits at x >= W are not pixels
        const uint32_t* mask = bits + m * H * W32;
        const uint32_t above0 = rle_above0(mask, W32, H, w);
        const int64_t off = offsets[m];
        // entries of this mask that may be written: its own T + 1, inside the buffer (a guard; the launcher has checked the capacity)
        const int64_t lim = max((int64_t)0, min(offsets[m + 1], capacity) - off);
        uint32_t* out = counts + off;
        uint32_t carry = 0u, my_rank = 0u, my_prev = 0u;           // lane c: column 32 w + c
        if (lane < ncols) {
            const int64_t i = m * W + 32 * w + lane;
            my_rank = rank[i];
            my_prev = prev[i];
        }
        for (int y0 = 0; y0 < H; y0 += 64) {
            const uint32_t t = rle_transitions(mask + w, W32, H, y0, lane, above0, carry);
            uint32_t cols = rle_active_columns(t, valid);
            while (cols) {                                         // wave-uniform
                const int c = __builtin_ctz(cols);
                cols &= cols - 1u;
                const unsigned long long b = __ballot((t >> c) & 1u);
                const uint32_t col_rank = (uint32_t)__builtin_amdgcn_readlane((int)my_rank, c);
                const uint32_t col_prev = (uint32_t)__builtin_amdgcn_readlane((int)my_prev, c);
                const uint32_t base = (uint32_t)(32 * w + c) * (uint32_t)H + (uint32_t)y0;
                if ((b >> lane) & 1ull) {
                    const unsigned long long below = b & below_me;
                    const uint32_t before = below ? base + (uint32_t)(63 - __clzll((long long)below)) : col_prev;
                    const int64_t k = (int64_t)col_rank + __popcll(below);
                    if (k < lim) out[k] = base + (uint32_t)lane - before;
                }
                if (lane == c) {
                    my_rank += (uint32_t)__popcll(b);
                    my_prev = base + (uint32_t)(63 - __clzll((long long)b));
                }
            }
        }
        // the closing run: from the mask's last transition to H W
        if (w == W32 - 1 && lane == ncols - 1 && (int64_t)my_rank < lim) out[my_rank] = (uint32_t)((int64_t)H * W) - my_prev;
    }
}

// ------------------------------------------------------------------------------------------------ decoder
__device__ __forceinline__ void rle_flip(uint32_t* __restrict__ mask, int W32, int H, uint64_t p) {
    const uint32_t x = (uint32_t)(p / (uint32_t)H), y = (uint32_t)(p - (uint64_t)x * (uint32_t)H);
    atomicXor(mask + (int64_t)y * W32 + (x >> 5), 1u << (x & 31));
}

__global__ __launch_bounds__(256) void rle_toggle_kernel(const uint32_t* __restrict__ counts, const int64_t* __restrict__ offsets, int H, int W, int W32,
                                                         uint32_t* __restrict__ bits) {
    __shared__ uint64_t sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t off = offsets[blockIdx.x], len = offsets[blockIdx.x + 1] - off;
    const uint64_t HW = (uint64_t)H * (uint64_t)W, per_word = (uint64_t)32 * (uint64_t)H;
    uint32_t* mask = bits + (int64_t)blockIdx.x * H * W32;
    uint64_t run = 0;                                              // pixels before this round's entries, at most H W
    for (int64_t k0 = 0; k0 < len && run < HW; k0 += 256) {        // block-uniform
        const int64_t k = k0 + (int64_t)threadIdx.x;
        const uint64_t v = k < len ? (uint64_t)counts[off + k] : 0ull;
        uint64_t s = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = __shfl_up(s, d, 64);
            if (lane >= d) s += o;
        }
        __syncthreads();
        if (lane == 63) sh[wave] = s;
        __syncthreads();
        uint64_t tot = 0;
#pragma unroll
        for (int v4 = 0; v4 < 4; ++v4) {
            if (v4 == wave) s += tot;
            tot += sh[v4];
        }
        if (k < len && (k & 1)) {                                  // a run of ones: pixels [a, e), clamped at H W (256 entries of 32 bits fit 64)
            const uint64_t e = min(run + s, HW), a = min(run + s - v, HW);
            if (a < e) {
                rle_flip(mask, W32, H, a);
                if (e < HW) rle_flip(mask, W32, H, e);
                // word columns w >= 1 whose first pixel follows a pixel of this run: a < 32 w H <= e
                for (uint64_t wc = a / per_word + 1; wc * per_word <= e && wc < (uint64_t)W32; ++wc) rle_flip(mask, W32, H, wc * per_word);
            }
        }
        run = min(run + tot, HW);
    }
}

__global__ __launch_bounds__(64 * RLE_WAVES) void rle_sweep_kernel(uint32_t* __restrict__ bits, int H, int W, int W32, int64_t pairs) {
    const int lane = threadIdx.x & 63;
    for (int64_t pair = (int64_t)blockIdx.x * RLE_WAVES + (threadIdx.x >> 6); pair < pairs; pair += (int64_t)gridDim.x * RLE_WAVES) {      // wave-uniform
        const int64_t m = pair / W32;
        const int w = (int)(pair - m * W32);
        const int ncols = min(32, W - 32 * w);
        const uint32_t valid = ncols == 32 ? 0xffffffffu : (1u << ncols) - 1u;
        uint32_t* col = bits + m * H * W32 + w;
        // parity of every column's flips
        uint32_t par = 0u;
        for (int y = lane; y < H; y += 64) par ^= col[(int64_t)y * W32];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) par ^= __shfl_xor(par, d, 64);
        // a column starts with the value the column before it ends with: the parity of the flips of the word's columns before it
        uint32_t start = par;
        start ^= start << 1; start ^= start << 2; start ^= start << 4; start ^= start << 8; start ^= start << 16;
        start <<= 1;
        for (int y0 = 0; y0 < H; y0 += 64) {
            const int y = y0 + lane;
            uint32_t v = y < H ? col[(int64_t)y * W32] : 0u;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(v, d, 64);
                if (lane >= d) v ^= o;
            }
            v ^= start;
            if (y < H) col[(int64_t)y * W32] = v & valid;
            start = __shfl(v, 63, 64);
        }
    }
}

// ------------------------------------------------------------------------------------------------ launchers
static const char* rle_shape_error(const char* who, int n, int H, int W, char* msg, size_t msg_len) {
    if (n < 1 || H < 1 || W < 1) {
        snprintf(msg, msg_len, "%s: n, H and W must be at least 1", who);
        return msg;
    }
    if ((int64_t)H * W >= ((int64_t)1 << 31)) {
        snprintf(msg, msg_len, "%s: masks of 2^31 pixels or more are not supported", who);
        return msg;
    }
    return nullptr;
}

size_t rle_workspace_bytes(int n, int H, int W) {
    if (n < 1 || H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return 0;
    return 2 * rle_align((size_t)n * (size_t)W * 4) + rle_align((size_t)n * 4);
}

static unsigned rle_pair_blocks(int64_t pairs) { return (unsigned)std::min<int64_t>((pairs + RLE_WAVES - 1) / RLE_WAVES, RLE_MAX_BLOCKS); }

static const char* rle_ws_error(const char* who, int n, int H, int W, const void* ws, size_t ws_bytes, char* msg, size_t msg_len) {
    if ((uintptr_t)ws & 15u) {
        snprintf(msg, msg_len, "%s: the workspace must be 16-byte aligned", who);
        return msg;
    }
    const size_t need = rle_workspace_bytes(n, H, W);
    if (ws_bytes < need) {
        snprintf(msg, msg_len, "%s: the workspace is too small (%zu bytes for %d masks of %d x %d)", who, need, n, H, W);
        return msg;
    }
    return nullptr;
}

const char* launch_rle_count(const uint32_t* bits, int n, int H, int W, int64_t* offsets, void* ws, size_t ws_bytes, hipStream_t s) {
    static thread_local char msg[160];
    if (const char* e = rle_shape_error("rle_count", n, H, W, msg, sizeof msg)) return e;
    if (!bits || !offsets || !ws) return "rle_count: null pointer";
    if (((uintptr_t)bits & 3u) || ((uintptr_t)offsets & 7u)) return "rle_count: bits must be 4-byte and offsets 8-byte aligned";
    if (const char* e = rle_ws_error("rle_count", n, H, W, ws, ws_bytes, msg, sizeof msg)) return e;
    const int W32 = (W + 31) / 32;
    const int64_t pairs = (int64_t)n * W32;
    const RleWs r = rle_carve(ws, n, W);
    hipLaunchKernelGGL(rle_colcount_kernel, dim3(rle_pair_blocks(pairs)), dim3(64 * RLE_WAVES), 0, s, bits, H, W, W32, pairs, r.rank, r.prev);
    hipLaunchKernelGGL(rle_colscan_kernel, dim3((unsigned)n), dim3(256), 0, s, r.rank, r.prev, r.total, W);
    hipLaunchKernelGGL(rle_offsets_kernel, dim3(1), dim3(256), 0, s, (const uint32_t*)r.total, n, offsets);
    return nullptr;
}

const char* launch_rle_encode(const uint32_t* bits, int n, int H, int W, const int64_t* offsets, uint32_t* counts, int64_t capacity, void* ws, size_t ws_bytes,
                              hipStream_t s) {
    static thread_local char msg[200];
    if (const char* e = rle_shape_error("rle_encode", n, H, W, msg, sizeof msg)) return e;
    if (!bits || !offsets || !counts || !ws) return "rle_encode: null pointer";
    if (((uintptr_t)bits & 3u) || ((uintptr_t)counts & 3u) || ((uintptr_t)offsets & 7u)) return "rle_encode: bits and counts must be 4-byte and offsets 8-byte aligned";
    if (const char* e = rle_ws_error("rle_encode", n, H, W, ws, ws_bytes, msg, sizeof msg)) return e;
    // the capacity is checked on the host: 8 bytes back, behind whatever the stream still holds (rle_count, as a rule long done)
    int64_t total = 0;
    hipError_t st = hipMemcpyAsync(&total, offsets + n, sizeof total, hipMemcpyDeviceToHost, s);
    if (st == hipSuccess) st = hipStreamSynchronize(s);
    if (st != hipSuccess) {
        snprintf(msg, sizeof msg, "rle_encode: reading offsets[n]: %s", hipGetErrorString(st));
        return msg;
    }
    if (total < n || capacity < total) {
        snprintf(msg, sizeof msg, "rle_encode: capacity %lld is below offsets[n] = %lld (or offsets do not come from rle_count)", (long long)capacity, (long long)total);
        return msg;
    }
    const int W32 = (W + 31) / 32;
    const int64_t pairs = (int64_t)n * W32;
    const RleWs r = rle_carve(ws, n, W);
    hipLaunchKernelGGL(rle_write_kernel, dim3(rle_pair_blocks(pairs)), dim3(64 * RLE_WAVES), 0, s, bits, H, W, W32, pairs, (const uint32_t*)r.rank,
                       (const uint32_t*)r.prev, offsets, counts, capacity);
    return nullptr;
}

const char* launch_rle_decode(const uint32_t* counts, const int64_t* offsets, int n, int H, int W, uint32_t* bits_out, hipStream_t s) {
    static thread_local char msg[160];
    if (const char* e = rle_shape_error("rle_decode", n, H, W, msg, sizeof msg)) return e;
    if (!counts || !offsets || !bits_out) return "rle_decode: null pointer";
    if (((uintptr_t)bits_out & 3u) || ((uintptr_t)counts & 3u) || ((uintptr_t)offsets & 7u)) return "rle_decode: bits and counts must be 4-byte and offsets 8-byte aligned";
    const int W32 = (W + 31) / 32;
    const int64_t pairs = (int64_t)n * W32;
    const hipError_t st = hipMemsetAsync(bits_out, 0, (size_t)n * H * W32 * 4, s);
    if (st != hipSuccess) {
        snprintf(msg, sizeof msg, "rle_decode: %s", hipGetErrorString(st));
        return msg;
    }
    hipLaunchKernelGGL(rle_toggle_kernel, dim3((unsigned)n), dim3(256), 0, s, counts, offsets, H, W, W32, bits_out);
    hipLaunchKernelGGL(rle_sweep_kernel, dim3(rle_pair_blocks(pairs)), dim3(64 * RLE_WAVES), 0, s, bits_out, H, W, W32, pairs);
    return nullptr;
}
