// Row-generic pieces of the fused token-side kernels: a workgroup of 8 waves owns 32 token rows in LDS (decoder_tokens.hip: 4 prompts x 8
// tokens; decoder_t16.hip: 2 prompts x 16 tokens) and streams the weights of every projection from L2 into MFMA operand registers.
// Included by both kernel files inside their operand-type namespace (op_wrap.hip).
#pragma once
#include "common.h"
#include "kernels.h"

#define TK_T 512               // threads per workgroup: 8 waves, two output tiles of 16 columns each per 256-wide projection
#define TK_R 32                // token rows per workgroup
#define TK_AS 528              // bytes per row of a bf16 operand buffer (256 + 8 elements: 16 rows x 16 B hit disjoint banks)
#define TK_FS 132              // floats per row of an fp32 scratch buffer (128 + 4)

struct TokCtx { int tid, lane, wave, fi, fg; char* Q; char* B0; char* B1; char* F0; char* F1; char* F2; char* H; };

// acc[i][m][r] = sum_k W[n0 + 16 (wave NTW + i) + 4 fg + r][k] * A[row 16 m + fi][k]  (W rows beyond nrows are clamped: their results are not used)
// Wpk (optional) = launch_pack_w_kstep's copy [K / 32][Npk][4 chunks, XOR-permuted by row][8] of the matrix whose row `row_off` is W's row 0: a
// 16 x 32 fragment is then one contiguous KB (eight full lines) instead of sixteen half lines of sixteen rows.
__device__ __forceinline__ int tk_perm(int row) { return (0x78 >> (((row >> 2) & 3) * 2)) & 3; }          // gemm_rowln.hip rl_perm
template <int NTW, int MT>
__device__ __forceinline__ void wgemm(const TokCtx& c, const char* A, int K, const bf16_t* W, int ldw, int n0, int nrows, f32x4 (&acc)[NTW][MT],
                                      const bf16_t* Wpk = nullptr, int Npk = 0, int row_off = 0) {
#pragma unroll
    for (int i = 0; i < NTW; ++i)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[i][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bf16_t* wr[NTW];
    int64_t kstride = 32;                   // elements from one K-step's fragment to the next
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int n = min(n0 + 16 * (c.wave * NTW + i) + c.fi, nrows - 1);
        if (Wpk) wr[i] = Wpk + (int64_t)(row_off + n) * 32 + ((c.fg ^ tk_perm(row_off + n)) << 3);
        else wr[i] = W + (int64_t)n * ldw + 8 * c.fg;
    }
    if (Wpk) kstride = (int64_t)Npk * 32;
#pragma unroll 8
    for (int ks = 0; ks < K / 32; ++ks) {
        op16x8 b[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) b[m] = *reinterpret_cast<const op16x8*>(A + (16 * m + c.fi) * TK_AS + (32 * ks + 8 * c.fg) * 2);
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const op16x8 a = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(wr[i] + ks * kstride));
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[i][m] = MFMA_16x16x32(a, b[m], acc[i][m], 0, 0, 0);
        }
    }
}

// The same product with the weight fragments of the whole call (K = 256: 8 k-steps x 2 column tiles = 64 registers) REQUESTED AHEAD: wfrag_load
// is issued one call early (the MLP walks 16 dependent 128-KB weight panels per segment, each behind a workgroup barrier: fetched inside the
// call, every panel paid an L2 round trip with nothing to overlap it - round 5).  Same MFMA order as wgemm: bit-identical results.
__device__ __forceinline__ void wfrag_load(const TokCtx& c, const bf16_t* Wpk, int N, int n0, int ks0, uint4 (&w)[2][8]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = n0 + 16 * (c.wave * 2 + i) + c.fi;
        const bf16_t* wr = Wpk + ((int64_t)ks0 * N + n) * 32 + ((c.fg ^ tk_perm(n)) << 3);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) w[i][ks] = *reinterpret_cast<const uint4*>(wr + (int64_t)ks * N * 32);
    }
    __builtin_amdgcn_sched_barrier(0);          // the requests stay HERE (ahead of the previous panel's MFMAs), not next to their use
}
__device__ __forceinline__ void wgemm_pre(const TokCtx& c, const char* A, const uint4 (&w)[2][8], f32x4 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[i][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        op16x8 b[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) b[m] = *reinterpret_cast<const op16x8*>(A + (16 * m + c.fi) * TK_AS + (32 * ks + 8 * c.fg) * 2);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const op16x8 a = __builtin_bit_cast(op16x8, w[i][ks]);
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[i][m] = MFMA_16x16x32(a, b[m], acc[i][m], 0, 0, 0);
        }
    }
}

// B = bf16(Q + (pe ? tok_pe : 0)) for the workgroup's 32 rows
__device__ __forceinline__ void to_operand(const TokCtx& c, char* B, const float* pe_rows /* global, this workgroup's first row, or null */, int rows_valid) {
    for (int idx = c.tid; idx < TK_R * 64; idx += TK_T) {
        const int r = idx >> 6, c4 = (idx & 63) * 4;
        float4 v = *reinterpret_cast<const float4*>(c.Q + (r * 256 + c4) * 4);
        if (pe_rows && r < rows_valid) {
            const float4 p = *reinterpret_cast<const float4*>(pe_rows + r * 256 + c4);
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        *reinterpret_cast<uint2*>(B + r * TK_AS + c4 * 2) = make_uint2(pack_op16(v.x, v.y), pack_op16(v.z, v.w));
    }
}
// Q[row] = LN(Q[row]) for the workgroup's 32 rows (wave w: rows 4 w .. 4 w + 3; a lane holds 4 channels)
__device__ __forceinline__ void ln_rows(const TokCtx& c, TokLn ln, float eps) {
    const float4 g = *reinterpret_cast<const float4*>(ln.g + 4 * c.lane), b = *reinterpret_cast<const float4*>(ln.b + 4 * c.lane);
    for (int r = 4 * c.wave; r < 4 * c.wave + 4; ++r) {
        float4* q = reinterpret_cast<float4*>(c.Q + (r * 256 + 4 * c.lane) * 4);
        const float4 v = *q;
        const float mean = wave_sum((v.x + v.y) + (v.z + v.w)) * (1.0f / 256.0f);
        const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
        const float rstd = 1.0f / sqrtf(wave_sum((a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3)) * (1.0f / 256.0f) + eps);
        *q = make_float4(a0 * rstd * g.x + b.x, a1 * rstd * g.y + b.y, a2 * rstd * g.z + b.z, a3 * rstd * g.w + b.w);
    }
}
// Q (+)= A . W^T + bias for N = 256 (residual: add to Q, else overwrite)
__device__ __forceinline__ void proj_to_q(const TokCtx& c, const char* A, int K, TokLin L, bool residual) {
    f32x4 acc[2][2];
    wgemm<2, 2>(c, A, K, L.w, L.ldw, 0, 256, acc, L.wpk, L.npk, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = 16 * (c.wave * 2 + i) + 4 * c.fg;
        const float4 b = *reinterpret_cast<const float4*>(L.b + n);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            float4* q = reinterpret_cast<float4*>(c.Q + ((16 * m + c.fi) * 256 + n) * 4);
            float4 v = make_float4(acc[i][m][0] + b.x, acc[i][m][1] + b.y, acc[i][m][2] + b.z, acc[i][m][3] + b.w);
            if (residual) { const float4 o = *q; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
            *q = v;
        }
    }
}
// F[row][0..127] = A . W[n0 .. n0+127]^T + bias (fp32 scratch, 128 columns)
__device__ __forceinline__ void proj_to_f(const TokCtx& c, const char* A, int K, TokLin L, int n0, char* F) {
    f32x4 acc[1][2];
    wgemm<1, 2>(c, A, K, L.w, L.ldw, n0, L.n, acc, L.wpk, L.npk, 0);
#pragma unroll
    for (int i = 0; i < 1; ++i) {
        const int n = 16 * (c.wave + i) + 4 * c.fg;
        const float4 b = *reinterpret_cast<const float4*>(L.b + n0 + n);
#pragma unroll
        for (int m = 0; m < 2; ++m)
            *reinterpret_cast<float4*>(F + ((16 * m + c.fi) * TK_FS + n) * 4) =
                make_float4(acc[i][m][0] + b.x, acc[i][m][1] + b.y, acc[i][m][2] + b.z, acc[i][m][3] + b.w);
    }
}
__device__ __forceinline__ op16x8 pack8(const float (&v)[8]) {
    const uint4 u = make_uint4(pack_op16(v[0], v[1]), pack_op16(v[2], v[3]), pack_op16(v[4], v[5]), pack_op16(v[6], v[7]));
    return __builtin_bit_cast(op16x8, u);
}
