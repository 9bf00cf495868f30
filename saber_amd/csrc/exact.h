// Launchers of the exact-precision (fp32) kernels (exact.hip), shared by the engine's exact mode and the kernel-level C-ABI
// (capi_kernels.hip: saber_k_xg_*).  Each returns nullptr or the message of an argument it refuses.
#pragma once
#include "engine.h"

// C[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) (+ res) per batch entry b (A + b sA, W + b sW, bias + b sBias, C + b sC)
struct XGemm {
    const float* A = nullptr; int64_t lda = 0; int64_t sA = 0;
    const float* W = nullptr; int64_t ldw = 0; int64_t sW = 0;
    const float* bias = nullptr; int64_t sBias = 0;
    const float* res = nullptr; int64_t ldres = 0; int res_shift = 0; int64_t res_mod = 0;
    // res_rows_per > 0: per-prompt rows against per-slot tables - the residual of row r is res[((r / res_rows_per + res_off) / res_div) * res_stride +
    // (r % res_rows_per) * ldres + n] (the xg_add_slot mapping folded into the epilogue)
    int64_t res_rows_per = 0, res_stride = 0; int res_div = 1, res_off = 0;
    // A2: the operand is A[m][k] + A2[(m % a2_mod)][k], summed in fp32 before the product exactly as a stored sum would be (keys + dense_pe)
    const float* A2 = nullptr; int64_t lda2 = 0; int64_t a2_mod = 1;
    int64_t row0 = 0;      // first row of this launch within the whole GEMM (row slabs): the A2 and slot-residual mappings count from there
    float* C = nullptr; int64_t ldc = 0; int64_t sC = 0;
    // pool4: output row q = max over rows 4q .. 4q+3, + bias; no activation, residual, act_last or A2 with it (refused)
    int M = 0, N = 0, K = 0, act = ACT_NONE, act_last = 0, pool4 = 0, batch = 1;
};

const char* xg_gemm(const XGemm& p, hipStream_t s);
const char* xg_layernorm(const float* x, const LnW& w, float eps, float* out, int64_t rows, int C, int act, hipStream_t s,
                         const uint8_t* row_valid = nullptr, int valid_mod = 0);
void xg_add(const float* x, const float* y, int64_t ymod, float* out, int64_t rows, int C, hipStream_t s);
void xg_add_slot(const float* in, const float* tab, XMap m, const float* vec, float* out, int64_t rows_per, int C, int P, int act, hipStream_t s);
const char* xg_attn(int hd, const float* q, int64_t q_bs, int ldq, const float* k, int64_t k_bs, int ldk, const float* v, int64_t v_bs, int ldv,
                    float* o, int64_t o_bs, int ldo, int nq, int nk, int batch, int heads, int qpool, const uint8_t* kmask, float scale, hipStream_t s);
// h2[p][tok][16] of the mask prompt's first two stages (conv k2s2 + LayerNorm2d + GELU, twice) for P planes of 256 x 256
void xg_mask_hidden(const float* mask_in, int P, const MaskEmbedWeights& w, float clamp_abs, int raw4_q0, float* h2out, hipStream_t s);
// masks4[p][k][y][x] = sum_c hyper[p][k][c] up[p][perm(y, x)][c]
void xg_mask_dot(const float* up, const float* hyper, int P, float* masks4, hipStream_t s);
