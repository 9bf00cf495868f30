// The MLP half of a Hiera MultiScaleBlock as ONE row-owner kernel: the hidden activation never leaves the compute unit.
//
//     h   = rnd16( GELU( xn[M,C] . W1[4C,C]^T + b1 ) )      (registers only)
//     y   = h . W2[C,4C]^T + b2 + res                        (fp32, written to Cf: the residual stream, in place over res)
//     xn' = LayerNorm(y) * gamma + beta                      (16-bit, written to ln_out: norm1 of the NEXT block)
//     [Cb = rnd16(y)]                                        (optional: the stage output that feeds the FPN neck)
//
// Replaces the pair mlp.layers.0 (launch_gemm, ACT_GELU, 16-bit out) -> mlp.layers.1 (gemm_rowln_kernel) of the stage-0 blocks, whose
// hidden tensor (tokens x 4C 16-bit values: 1.6 GB per block on the 21-crop pass) was written to HBM by one launch and read back by the next.
// Same arithmetic as the pair: fp32 accumulation with 16x16x32 MFMAs over ascending K from a zero accumulator, bias added in fp32,
// gelu_erf2 on the same value pairs, h rounded with pack_op16, the second product over ascending hidden index, then the shared epilogue
// (rowln_epilogue.h) - the pair's results, bit for bit.
//
//   * a wave owns 32 whole rows (workgroup: 8 waves, tile = 256 rows): its xn rows stay in registers for the tile (2 x 5 operand
//     fragments, the K tail 144..159 zeroed), its y rows are 2 x 9 accumulator tiles (72 registers).
//   * the hidden dimension is walked in chunks of 32 = one K-step of the second product.  Per chunk: 2 x 2 tiles of the first product
//     (20 MFMAs), bias + GELU + pack in registers, 18 MFMAs of the second.  NO transposition in between: the first product is computed as
//     W1 . xn^T, which leaves lane (fi, fg) with row fi and the four hidden columns fg * 4 .. + 3 of a 16-column tile, and the second product
//     wants row fi with the eight hidden values fg * 8 .. + 7 of the K-step - so the packed W1 puts hidden column 32 s + 8 g + 4 j + r of chunk s
//     into row 4 g + r of tile j, and the two tiles' registers ARE the operand (pack_mlp_chunks_kernel).
//   * weights stream L2 -> registers -> LDS one chunk ahead (two buffers of 19 KB, one barrier per chunk), packed once per weight as the
//     sequence of 1-KB MFMA fragments the waves read, each fragment lane-linear (lane l's 16 B at byte 16 l: conflict-free ds_read_b128,
//     full-line global loads).  Ordinary loads and __syncthreads(): every wait in the main loop is the compiler's.
//   * persistent: min(tiles, CUs) workgroups walk the row tiles; the next tile's xn rows are requested from the middle of the epilogue.
// A row's result depends on nothing but that row: not on M, the tile or the workgroup.
#include "common.h"
#include "kernels.h"
#include "rowln_epilogue.h"

#define ML_HC 32                     // hidden columns per chunk

template <int C> struct MlpRowLnCfg {
    // (the row-owner layout of rowln_epilogue.h is 144 columns per wave: C = 288 would need two waves per row, which shares h between waves
    // through LDS and halves the rows per tile against four times the weight bytes - DESIGN.md section 8.1)
    static_assert(C == 144, "built for the stage-0 width");
    static constexpr int R = 256;
    static constexpr int NK1 = (C + 31) / 32;                 // K-steps of the first product
    static constexpr int NT = C / 16;                         // column tiles of the second
    static constexpr int FR = 2 * NK1 + NT;                   // 1-KB fragments per chunk: W1 tile j, K-step ks at j NK1 + ks; W2 column tile nt at 2 NK1 + nt
    static constexpr int NCH = 4 * C / ML_HC;
    static constexpr int CHUNK = FR * 1024;
    static constexpr int UNITS = CHUNK / 16, NU = (UNITS + 511) / 512;      // 16-B units of a chunk, per thread
    static constexpr int BUF = NU * 512 * 16;                 // LDS buffer of a chunk: every thread writes NU units, the surplus ones behind the chunk
    static constexpr int B1_OFF = 2 * BUF;                    // b1 as fp32
    static constexpr int SCR_OFF = B1_OFF + 4 * C * 4;        // transposition scratch of the epilogue
    static constexpr int LDS = SCR_OFF + 8 * RL_SCR;
};

template <int C>
__global__ __launch_bounds__(512) void gemm_rowln_mlp_kernel(GemmParams p) {
    using CF = MlpRowLnCfg<C>;
    constexpr int R = CF::R, NK1 = CF::NK1, NT = CF::NT, NCH = CF::NCH, NU = CF::NU;
    static_assert(NT == 9, "rowln_epilogue: 9 column tiles per wave");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fi = lane & 15, fg = lane >> 4;
    const int tiles = (p.M + R - 1) / R;
    int tl = blockIdx.x;                                   // position in this workgroup's walk
    if (tl >= tiles) return;
    auto tile_of = [&](int l) { return p.rev ? tiles - 1 - l : l; };

    float* b1s = reinterpret_cast<float*>(smem + CF::B1_OFF);
    for (int i = tid; i < 4 * C; i += 512) b1s[i] = p.bias1 ? p.bias1[i] : 0.f;

    // weight chunks: a straight copy of CHUNK bytes, unit u = tid + 512 q (the surplus units of the last round repeat the chunk's last one and
    // land behind it).  No condition on either side: a conditional write lets hipcc sink its load into the branch, behind the chunk's MFMAs,
    // where the L2 latency is exposed once per chunk; the scheduling barrier behind stage_load() keeps the loads at the top for the same reason.
    const u32x4* __restrict__ wsrc = reinterpret_cast<const u32x4*>(p.Wpk);
    u32x4 st[NU];
    auto stage_load = [&](int ch) {
#pragma unroll
        for (int q = 0; q < NU; ++q) st[q] = wsrc[(int64_t)ch * CF::UNITS + min(tid + 512 * q, CF::UNITS - 1)];
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NU; ++q) *reinterpret_cast<u32x4*>(smem + buf * CF::BUF + (tid + 512 * q) * 16) = st[q];
    };
    // this wave's xn rows as operand fragments: row wave * 32 + i * 16 + fi, k = ks * 32 + fg * 8 .. + 7; through a buffer descriptor over the
    // tile's rows (rows beyond M read as zero), k >= C zeroed
    op16x8 xn[2][NK1];
    auto load_xn = [&](int tile) {
        const int rows = min(R, p.M - tile * R);
        const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + (int64_t)tile * R * p.lda), 0, (int)((uint32_t)rows * (uint32_t)p.lda * 2u), 0x00020000);
        const uint32_t voff = (uint32_t)(((wave * 32 + fi) * (int)p.lda + fg * 8) * 2);
        const uint32_t istep = (uint32_t)(16 * (int)p.lda * 2);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int ks = 0; ks < NK1; ++ks) {
                u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(arsrc, voff + ks * 64, i * istep, 0);
                if ((ks + 1) * 32 > C && ks * 32 + fg * 8 >= C) v = (u32x4){0u, 0u, 0u, 0u};
                xn[i][ks] = __builtin_bit_cast(op16x8, v);
            }
    };

    stage_load(0);
    load_xn(tile_of(tl));
    stage_write(0);
    __syncthreads();
    int cur = 0;
    for (; tl < tiles; tl += gridDim.x) {
        const int m0 = tile_of(tl) * R;
        f32x4 acc[2][9];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 9; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int s = 0; s < NCH; ++s) {
            stage_load(s + 1 == NCH ? 0 : s + 1);         // (the walk's last chunk fetches chunk 0 for nobody: 19 KB from L2)
            __builtin_amdgcn_sched_barrier(0);
            const char* wb = smem + cur * CF::BUF + lane * 16;
            f32x4 h[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i) { h[i][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; h[i][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int ks = 0; ks < NK1; ++ks) {
                const op16x8 w0 = *reinterpret_cast<const op16x8*>(wb + ks * 1024), w1 = *reinterpret_cast<const op16x8*>(wb + (NK1 + ks) * 1024);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    h[i][0] = MFMA_16x16x32(w0, xn[i][ks], h[i][0], 0, 0, 0);
                    h[i][1] = MFMA_16x16x32(w1, xn[i][ks], h[i][1], 0, 0, 0);
                }
            }
            // lane (fi, fg) holds row fi, hidden columns 32 s + 8 fg + 4 j + r: bias, GELU and rounding as the ACT_GELU epilogue of gemm.hip
            const f32x4 ba = *reinterpret_cast<const f32x4*>(b1s + s * ML_HC + fg * 8), bb = *reinterpret_cast<const f32x4*>(b1s + s * ML_HC + fg * 8 + 4);
            op16x8 hf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const f32x2 g0 = gelu_erf2((f32x2){h[i][0][0] + ba[0], h[i][0][1] + ba[1]}), g1 = gelu_erf2((f32x2){h[i][0][2] + ba[2], h[i][0][3] + ba[3]});
                const f32x2 g2 = gelu_erf2((f32x2){h[i][1][0] + bb[0], h[i][1][1] + bb[1]}), g3 = gelu_erf2((f32x2){h[i][1][2] + bb[2], h[i][1][3] + bb[3]});
                const u32x4 u = {pack_op16(g0.x, g0.y), pack_op16(g1.x, g1.y), pack_op16(g2.x, g2.y), pack_op16(g3.x, g3.y)};
                hf[i] = __builtin_bit_cast(op16x8, u);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const op16x8 w2 = *reinterpret_cast<const op16x8*>(wb + (2 * NK1 + nt) * 1024);
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i][nt] = MFMA_16x16x32(w2, hf[i], acc[i][nt], 0, 0, 0);
            }
            stage_write(cur ^ 1);      // read last in chunk s - 1: every wave is past that chunk's barrier
            __syncthreads();
            cur ^= 1;
        }
        rowln_epilogue<2, 1, R>(p, acc, m0, wave, 0, wave, lane, static_cast<float*>(nullptr), smem + CF::SCR_OFF, [&] {
            // (unconditional - the walk's last tile re-reads its own rows for nobody: around loads in a branch hipcc waits for each one by itself)
            load_xn(tile_of(tl + (int)gridDim.x < tiles ? tl + (int)gridDim.x : tl));
        });
    }
}

// out[chunk s][fragment f][lane l][8]: the operand fragments in the order and lane layout the kernel reads them (see the file header).
// W1 [4C][ldw1], W2 [C][ldw2], rows zero-padded; k >= C of W1 packs as zero.
__global__ __launch_bounds__(256) void pack_mlp_chunks_kernel(const bf16_t* __restrict__ W1, int ldw1, const bf16_t* __restrict__ W2, int ldw2, int C, bf16_t* __restrict__ out) {
    const int nk1 = (C + 31) / 32, nt = C / 16, fr = 2 * nk1 + nt, nch = 4 * C / ML_HC;
    const int total = nch * fr * 64;                    // 16-B units
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int l = idx & 63, f = (idx >> 6) % fr, s = (idx >> 6) / fr;
        const int fi = l & 15, fg = l >> 4;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (f < 2 * nk1) {
            const int j = f / nk1, ks = f % nk1;
            const int row = s * ML_HC + (fi >> 2) * 8 + j * 4 + (fi & 3), k = ks * 32 + fg * 8;
            if (k < C) v = *reinterpret_cast<const uint4*>(W1 + (int64_t)row * ldw1 + k);
        } else {
            const int n = (f - 2 * nk1) * 16 + fi, k = s * ML_HC + fg * 8;
            v = *reinterpret_cast<const uint4*>(W2 + (int64_t)n * ldw2 + k);
        }
        *reinterpret_cast<uint4*>(out + (int64_t)idx * 8) = v;
    }
}

bool gemm_mlp_rowln_width(int C) { return C == 144; }
size_t gemm_mlp_rowln_packed_elems(int C) { return (size_t)(4 * C / ML_HC) * (2 * ((C + 31) / 32) + C / 16) * 512; }
const char* launch_pack_mlp_chunks(const bf16_t* W1, int ldw1, const bf16_t* W2, int ldw2, int C, bf16_t* out, hipStream_t s) {
    if (!gemm_mlp_rowln_width(C)) return "pack_mlp_chunks: width not built (144)";
    if ((ldw1 & 7) || ldw1 < C || (ldw2 & 7) || ldw2 < 4 * C) return "pack_mlp_chunks: ldw1 / ldw2 must be multiples of 8 and cover the rows";
    if (((uintptr_t)W1 & 15) || ((uintptr_t)W2 & 15) || ((uintptr_t)out & 15)) return "pack_mlp_chunks: operand alignment";
    const int total = (int)(gemm_mlp_rowln_packed_elems(C) / 8);
    hipLaunchKernelGGL(pack_mlp_chunks_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, W1, ldw1, W2, ldw2, C, out);
    return nullptr;
}

const char* gemm_mlp_rowln_init_device() {
    const hipError_t st = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_rowln_mlp_kernel<144>), hipFuncAttributeMaxDynamicSharedMemorySize, MlpRowLnCfg<144>::LDS);
    return st == hipSuccess ? nullptr : hipGetErrorString(st);
}

// p: A = xn [M][lda], N = K = C, Wpk = the launch_pack_mlp_chunks copy of (W1, W2), bias1 = b1, bias = b2, res / Cf / Cb / ln_* as launch_gemm_rowln
const char* launch_gemm_mlp_rowln(const GemmParams& p_in, hipStream_t stream) {
    GemmParams p = p_in;
    p.dbg = g_saber_debug_flags;
    if (!gemm_mlp_rowln_width(p.N) || p.K != p.N || !p.Wpk || !p.Cf || !p.ln_out || !p.ln_gamma || !p.ln_beta || p.batch > 1 || p.pool4 || p.act != ACT_NONE ||
        p.res_shift || p.res_mod)
        return "gemm_mlp_rowln: unsupported problem (C must be 144; packed weights, fp32 + LayerNorm outputs required)";
    if (p.M <= 0) return "gemm_mlp_rowln: empty problem";
    if (p.lda & 7) return "gemm_mlp_rowln: lda must be a multiple of 8";
    if (((uintptr_t)p.A & 15) || ((uintptr_t)p.Wpk & 15) || ((uintptr_t)p.Cf & 15) || (p.ldcf & 3) || ((uintptr_t)p.ln_out & 7) || (p.ldln & 3) ||
        (p.res && (((uintptr_t)p.res & 15) || (p.ldres & 3))) || (p.bias && ((uintptr_t)p.bias & 15)) || (p.bias1 && ((uintptr_t)p.bias1 & 3)) ||
        (p.Cb && (((uintptr_t)p.Cb & 7) || (p.ldcb & 3))) || ((uintptr_t)p.ln_gamma & 15) || ((uintptr_t)p.ln_beta & 15))
        return "gemm_mlp_rowln: operand alignment";
    if ((int64_t)p.M * p.lda >= ((int64_t)1 << 40)) return "gemm_mlp_rowln: problem too large";
    const int n_cu = saber_cu_count();
    const int tiles = (p.M + MlpRowLnCfg<144>::R - 1) / MlpRowLnCfg<144>::R;
    hipLaunchKernelGGL((gemm_rowln_mlp_kernel<144>), dim3(tiles < n_cu ? tiles : n_cu), dim3(512), MlpRowLnCfg<144>::LDS, stream, p);
    return nullptr;
}
