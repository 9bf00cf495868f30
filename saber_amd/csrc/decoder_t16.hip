// The 16-token route of the 16-bit decoder: prompts of 2..9 points (clicks, a box's two corners, a box plus clicks).
//
// A prompt of K points has 7 + K decoder tokens ([obj, iou, mask0..3, K points, padding point]); the 8-token kernels carry exactly 8.  Here
// a prompt carries 16 token rows [obj, iou, mask0..3, K points, padding point, zero rows]: rows 7 + K .. 15 are zero tokens with zero
// positional encoding (finite through every layer: a LayerNorm maps them to its beta) and every attention over the tokens masks them as keys.
//   token side      dec_tokens16_kernel: dec_tokens_kernel's segments with 2 prompts x 16 rows per workgroup (the same 32 rows, so the
//                   weight-streaming projections are unchanged), a 16 x 16 self attention per head with the padding keys masked, and the
//                   folds of the cross attentions in the layouts below
//   tokens -> image each query row is its own softmax over the image keys: a 16-token prompt runs as two 8-token "half prompts" over the
//                   same X through the unchanged dec_t2i kernels (fold_q in [P][2][64][256] order; tq / t_att rows are already in that order)
//   image -> tokens dec_i2t16_kernel: dec_i2t_kernel<1> with 128 score columns (c = 16 h + t) and the softmax over the 16 tokens of a head
//                   (columns t >= 7 + K get exactly zero weight)
#include "common.h"
#include "kernels.h"
#include "decoder_tokens.h"
#include <utility>

#define T16_C 256
#define T16_G 2                // prompts per token-side workgroup (TK_R = 16 T16_G rows)

// ------------------------------------------------------------------------------------------------ prompt tokens
// tokens[p] = [obj, iou, mask0..3, point(p, 0) .. point(p, K - 1), pad, zero rows]  (16 x 256 fp32; prompt_tokens_multi_kernel's arithmetic)
__global__ __launch_bounds__(256) void prompt_tokens16_kernel(const float* __restrict__ pts, const int* __restrict__ labels, int K, PromptWeights w,
                                                              float* __restrict__ tokens) {
    const int p = blockIdx.x, c = threadIdx.x;
    float* t = tokens + (int64_t)p * 16 * T16_C;
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k * T16_C + c] = w.out_tokens[k * T16_C + c];
    for (int k = 0; k < K; ++k) {
        const int label = labels[p * K + k];
        float e;
        if (label >= 0) {
            const float x = 2.0f * ((pts[2 * (p * K + k)] + 0.5f) / 1024.0f) - 1.0f;
            const float y = 2.0f * ((pts[2 * (p * K + k) + 1] + 0.5f) / 1024.0f) - 1.0f;
            const int f = c & 127;
            const float a = 6.283185307179586f * (x * w.gauss[f] + y * w.gauss[128 + f]);
            e = (c < 128 ? sinf(a) : cosf(a)) + w.point_embed[(label & 3) * T16_C + c];
        } else {
            e = w.not_a_point[c];
        }
        t[(6 + k) * T16_C + c] = e;
    }
    t[(6 + K) * T16_C + c] = w.not_a_point[c];
    for (int k = 7 + K; k < 16; ++k) t[k * T16_C + c] = 0.f;
}
const char* launch_prompt_tokens16(const float* pts, const int* labels, int P, int K, PromptWeights w, float* tokens, hipStream_t s) {
    if (P <= 0) return nullptr;
    if (K < 2 || K > 9 || !labels) return "prompt_tokens16: 2..9 points per prompt, with labels";
    hipLaunchKernelGGL(prompt_tokens16_kernel, dim3(P), dim3(256), 0, s, pts, labels, K, w, tokens);
    return nullptr;
}

// ------------------------------------------------------------------------------------------------ token side
// bf16 hi / lo block-diagonal operand of a fold (decoder_tokens.hip fold_operand) for the 8 tokens of rows row0 .. row0 + 7:
// row (hsel, t) = fi, k = 8 fg .. + 7 of [head 2 hp | head 2 hp + 1]
__device__ __forceinline__ void fold_operand16(const TokCtx& c, const char* F, int row0, int hp, float scale, op16x8* hi, op16x8* lo) {
    const int hsel = c.fi >> 3, t = c.fi & 7, hk = c.fg >> 1;
    const float* a = reinterpret_cast<const float*>(F) + (row0 + t) * TK_FS + 16 * (2 * hp + hsel) + 8 * (c.fg & 1);
    const float z = hk == hsel ? scale : 0.f;
    float v[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = a[j] * z;
        l[j] = v[j] - op2f(f2op(v[j]));
    }
    *hi = pack8(v); *lo = pack8(l);
}
// scale sum_j a[t][16 h + j] W(16 h + j, d), W given TRANSPOSED as WT bf16 [256][128] (decoder_tokens.hip fold_rows) written to
//   I2T = false: out[2 p + half][8 h + (t & 7)][d]    (the tokens -> image queries of two half prompts, half = t >> 3)
//   I2T = true:  out[p][16 h + t][d]                  (the image -> tokens keys of dec_i2t16)
template <bool I2T>
__device__ __forceinline__ void fold_rows16(const TokCtx& c, const char* F, const bf16_t* WT, float scale, bf16_t* out, int p0, int P) {
    op16x8 w[4][2];
#pragma unroll
    for (int hp = 0; hp < 4; ++hp)
#pragma unroll
        for (int i = 0; i < 2; ++i)
            w[hp][i] = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(WT + (16 * (c.wave * 2 + i) + c.fi) * 128 + 32 * hp + 8 * c.fg));
    for (int pi = 0; pi < T16_G; ++pi) {
        if (p0 + pi >= P) break;
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int hp = 0; hp < 4; ++hp) {
                op16x8 hi, lo;
                fold_operand16(c, F, 16 * pi + 8 * half, hp, scale, &hi, &lo);
                const int h = 2 * hp + (c.fi >> 3), t = c.fi & 7;
                const int64_t row = I2T ? (int64_t)(p0 + pi) * 128 + 16 * h + 8 * half + t : ((int64_t)(p0 + pi) * 2 + half) * 64 + 8 * h + t;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int dt = c.wave * 2 + i;
                    f32x4 acc = MFMA_16x16x32(w[hp][i], hi, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    acc = MFMA_16x16x32(w[hp][i], lo, acc, 0, 0, 0);
                    // D[d = 16 dt + 4 fg + r][(hsel, t) = fi]
                    bf16_t* o = out + row * 256 + 16 * dt + 4 * c.fg;
                    *reinterpret_cast<uint2*>(o) = make_uint2(pack_op16(acc[0], acc[1]), pack_op16(acc[2], acc[3]));
                }
            }
        }
    }
}
// out[p][d][16 h + t] = sum_j a[t][16 h + j] W[d][16 h + j], W bf16 [256][128] (decoder_tokens.hip fold_cols; 128 columns per row)
__device__ __forceinline__ void fold_cols16(const TokCtx& c, const char* F, const bf16_t* W, int ldw, bf16_t* out, int p0, int P) {
    op16x8 w[4][2];
#pragma unroll
    for (int hp = 0; hp < 4; ++hp)
#pragma unroll
        for (int i = 0; i < 2; ++i)
            w[hp][i] = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(W + (int64_t)(16 * (c.wave * 2 + i) + c.fi) * ldw + 32 * hp + 8 * c.fg));
    for (int pi = 0; pi < T16_G; ++pi) {
        if (p0 + pi >= P) break;
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int hp = 0; hp < 4; ++hp) {
                op16x8 hi, lo;
                fold_operand16(c, F, 16 * pi + 8 * half, hp, 1.0f, &hi, &lo);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int dt = c.wave * 2 + i;
                    f32x4 acc = MFMA_16x16x32(hi, w[hp][i], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    acc = MFMA_16x16x32(lo, w[hp][i], acc, 0, 0, 0);
                    // D[(hsel, t & 7) = 4 fg + r][d = 16 dt + fi]  ->  columns 16 (2 hp + hsel) + 8 half + (t & 7) of row d
                    bf16_t* o = out + ((int64_t)(p0 + pi) * 256 + 16 * dt + c.fi) * 128 + 32 * hp + 16 * (c.fg >> 1) + 8 * half + 4 * (c.fg & 1);
                    *reinterpret_cast<uint2*>(o) = make_uint2(pack_op16(acc[0], acc[1]), pack_op16(acc[2], acc[3]));
                }
            }
        }
    }
}

// dec_tokens_kernel (decoder_tokens.hip) for 16-token prompts: two prompts per workgroup; nvalid = 7 + K tokens of a prompt take part in the
// attentions as keys.  The fold outputs: fold_q [P][2][64][256] (two half prompts), fold_k [P][128][256], fold_cb [P][128], fold_v [P][256][128].
__global__ __launch_bounds__(TK_T) void dec_tokens16_kernel(TokSeg s, int nvalid) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TokCtx c;
    c.tid = threadIdx.x; c.lane = c.tid & 63; c.wave = __builtin_amdgcn_readfirstlane(c.tid >> 6); c.fi = c.lane & 15; c.fg = c.lane >> 4;
    c.Q = smem; c.B0 = c.Q + TK_R * 256 * 4; c.B1 = c.B0 + TK_R * TK_AS; c.H = c.B1 + TK_R * TK_AS;
    c.F0 = c.H + TK_R * TK_AS; c.F1 = c.F0 + TK_R * TK_FS * 4; c.F2 = c.F1 + TK_R * TK_FS * 4;
    const int p0 = blockIdx.x * T16_G;
    const int np = min(T16_G, s.P - p0), rows = 16 * np;
    const int64_t row0 = (int64_t)p0 * 16;
    const float* pe = s.tok_pe + row0 * 256;
    for (int idx = c.tid; idx < TK_R * 64; idx += TK_T) {
        const int r = idx >> 6, c4 = (idx & 63) * 4;
        *reinterpret_cast<float4*>(c.Q + (r * 256 + c4) * 4) = r < rows ? *reinterpret_cast<const float4*>(s.queries + (row0 + r) * 256 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ---------------- (1) output projection of the tokens -> image attention that has just run (t_att rows: half prompts = token order)
    if (s.t_att) {
        for (int idx = c.tid; idx < TK_R * 16; idx += TK_T) {
            const int r = idx >> 4, c8 = (idx & 15) * 8;
            *reinterpret_cast<uint4*>(c.B1 + r * TK_AS + c8 * 2) = r < rows ? *reinterpret_cast<const uint4*>(s.t_att + (row0 + r) * 128 + c8) : make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        proj_to_q(c, c.B1, 128, s.att_o, true);
        __syncthreads();
        ln_rows(c, s.att_ln, s.att_eps);
    }
    __syncthreads();
    // ---------------- (2) MLP, LN3, operands of the image -> tokens attention
    if (s.do_mlp) {
        to_operand(c, c.B0, nullptr, rows);
        __syncthreads();
        f32x4 acc2[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int m = 0; m < 2; ++m) acc2[i][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
        uint4 w1f[2][8], w2f[2][8];
        wfrag_load(c, s.mlp1_pk, 2048, 0, 0, w1f);
#pragma unroll 1
        for (int ch = 0; ch < 8; ++ch) {
            f32x4 acc[2][2];
            wfrag_load(c, s.mlp2_pk, 256, 0, 8 * ch, w2f);
            wgemm_pre(c, c.B0, w1f, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int n = 16 * (c.wave * 2 + i) + 4 * c.fg;
                const float4 b = *reinterpret_cast<const float4*>(s.mlp1.b + 256 * ch + n);
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    *reinterpret_cast<uint2*>(c.H + (16 * m + c.fi) * TK_AS + n * 2) =
                        make_uint2(pack_op16(fmaxf(acc[i][m][0] + b.x, 0.f), fmaxf(acc[i][m][1] + b.y, 0.f)), pack_op16(fmaxf(acc[i][m][2] + b.z, 0.f), fmaxf(acc[i][m][3] + b.w, 0.f)));
            }
            if (ch + 1 < 8) wfrag_load(c, s.mlp1_pk, 2048, 256 * (ch + 1), 0, w1f);
            __syncthreads();
            f32x4 part[2][2];
            wgemm_pre(c, c.H, w2f, part);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int m = 0; m < 2; ++m) acc2[i][m] += part[i][m];
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = 16 * (c.wave * 2 + i) + 4 * c.fg;
            const float4 b = *reinterpret_cast<const float4*>(s.mlp2.b + n);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                float4* q = reinterpret_cast<float4*>(c.Q + ((16 * m + c.fi) * 256 + n) * 4);
                const float4 o = *q;
                *q = make_float4(o.x + acc2[i][m][0] + b.x, o.y + acc2[i][m][1] + b.y, o.z + acc2[i][m][2] + b.z, o.w + acc2[i][m][3] + b.w);
            }
        }
        __syncthreads();
        ln_rows(c, s.ln3, 1e-5f);
        __syncthreads();
        to_operand(c, c.B0, pe, rows);
        to_operand(c, c.B1, nullptr, rows);
        __syncthreads();
        proj_to_f(c, c.B0, 256, s.i2t_k, 0, c.F0);
        proj_to_f(c, c.B1, 256, s.i2t_v, 0, c.F1);
        __syncthreads();
        for (int idx = c.tid; idx < rows * 32; idx += TK_T) {
            const int r = idx >> 5, c4 = (idx & 31) * 4;
            *reinterpret_cast<float4*>(s.tk_out + (row0 + r) * 128 + c4) = *reinterpret_cast<const float4*>(c.F0 + (r * TK_FS + c4) * 4);
        }
        if (c.tid < 128 * np) {      // cb[p][16 h + t] = scale sum_j k[t][16 h + j] b_q[16 h + j]
            const int pi = c.tid >> 7, h = (c.tid >> 4) & 7, t = c.tid & 15;
            const float* a = reinterpret_cast<const float*>(c.F0) + (16 * pi + t) * TK_FS + 16 * h;
            float acc = 0.f;
            for (int j = 0; j < 16; ++j) acc += a[j] * s.i2t_qb[16 * h + j];
            s.fold_cb[(int64_t)(p0 + pi) * 128 + 16 * h + t] = acc * s.kscale;
        }
        fold_rows16<true>(c, c.F0, s.i2t_qT, s.kscale, s.fold_k, p0, s.P);
        fold_cols16(c, c.F1, s.i2t_o, 128, s.fold_v, p0, s.P);
        __syncthreads();
    }
    // ---------------- (3) self attention of the tokens: 16 x 16 per head, keys >= nvalid masked
    if (s.do_self) {
        if (!s.do_mlp) {
            to_operand(c, c.B0, s.self_first ? nullptr : pe, rows);
            if (!s.self_first) to_operand(c, c.B1, nullptr, rows);
            __syncthreads();
        }
        const char* xv = s.self_first ? c.B0 : c.B1;
        for (int hc = 0; hc < 2; ++hc) {             // heads 4 hc .. 4 hc + 3 (128 columns)
            proj_to_f(c, c.B0, 256, s.sa_q, 128 * hc, c.F0);
            proj_to_f(c, c.B0, 256, s.sa_k, 128 * hc, c.F1);
            proj_to_f(c, xv, 256, s.sa_v, 128 * hc, c.F2);
            __syncthreads();
            if (c.tid < 64 * T16_G) {
                const int pi = c.tid >> 6, hh = (c.tid >> 4) & 3, qi = c.tid & 15;
                const float* qp = reinterpret_cast<const float*>(c.F0) + (16 * pi + qi) * TK_FS + 32 * hh;
                float qv[32];
#pragma unroll
                for (int d = 0; d < 32; ++d) qv[d] = qp[d];
                const float scale = rsqrtf(32.0f);
                float sc[16], mx = -3.0e38f;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const float* kp = reinterpret_cast<const float*>(c.F1) + (16 * pi + j) * TK_FS + 32 * hh;
                    float a = 0.f;
#pragma unroll
                    for (int d = 0; d < 32; ++d) a += qv[d] * kp[d];
                    sc[j] = a * scale;
                    if (j < nvalid) mx = fmaxf(mx, sc[j]);
                }
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) { sc[j] = j < nvalid ? expf(sc[j] - mx) : 0.f; sum += sc[j]; }
                const float inv = 1.0f / sum;
                float o[32];
#pragma unroll
                for (int d = 0; d < 32; ++d) o[d] = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if (j >= nvalid) break;
                    const float* vp = reinterpret_cast<const float*>(c.F2) + (16 * pi + j) * TK_FS + 32 * hh;
                    const float pj = sc[j] * inv;
#pragma unroll
                    for (int d = 0; d < 32; ++d) o[d] += pj * vp[d];
                }
                char* op = c.H + (16 * pi + qi) * TK_AS + (128 * hc + 32 * hh) * 2;
#pragma unroll
                for (int d = 0; d < 32; d += 4) *reinterpret_cast<uint2*>(op + d * 2) = make_uint2(pack_op16(o[d], o[d + 1]), pack_op16(o[d + 2], o[d + 3]));
            }
            __syncthreads();
        }
        proj_to_q(c, c.H, 256, s.sa_o, !s.self_first);
        __syncthreads();
        ln_rows(c, s.ln1, 1e-5f);
        __syncthreads();
    }
    // ---------------- (4) operands of the next tokens -> image attention, folded for two half prompts per prompt
    if (s.do_t2i) {
        to_operand(c, c.B0, pe, rows);
        __syncthreads();
        proj_to_f(c, c.B0, 256, s.t2i_q, 0, c.F0);
        __syncthreads();
        for (int idx = c.tid; idx < rows * 32; idx += TK_T) {
            const int r = idx >> 5, c4 = (idx & 31) * 4;
            *reinterpret_cast<float4*>(s.tq_out + (row0 + r) * 128 + c4) = *reinterpret_cast<const float4*>(c.F0 + (r * TK_FS + c4) * 4);
        }
        fold_rows16<false>(c, c.F0, s.t2i_kT, s.kscale, s.fold_q, p0, s.P);
    }
    __syncthreads();
    for (int idx = c.tid; idx < rows * 64; idx += TK_T) {
        const int r = idx >> 6, c4 = (idx & 63) * 4;
        *reinterpret_cast<float4*>(s.queries + (row0 + r) * 256 + c4) = *reinterpret_cast<const float4*>(c.Q + (r * 256 + c4) * 4);
    }
    // ---------------- (5) heads on the final tokens (rows 0..5 of each prompt, at a stride of 16 rows)
    if (s.do_heads) {
        auto mlp3 = [&](const TokLin* L, int64_t w_off0, int64_t w_off2, int r_off0, int r_off2, int b_off0, int b_off2, int token, int n_out, int sigmoid, float* out, int ldo, int o_off) {
            for (int idx = c.tid; idx < 16 * 64; idx += TK_T) {
                const int r = idx >> 6, c4 = (idx & 63) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < np) v = *reinterpret_cast<const float4*>(c.Q + ((16 * r + token) * 256 + c4) * 4);
                *reinterpret_cast<uint2*>(c.B0 + r * TK_AS + c4 * 2) = make_uint2(pack_op16(v.x, v.y), pack_op16(v.z, v.w));
            }
            __syncthreads();
            for (int l = 0; l < 2; ++l) {
                const char* in = l == 0 ? c.B0 : c.B1;
                char* outb = l == 0 ? c.B1 : c.H;
                f32x4 acc[2][1];
                wgemm<2, 1>(c, in, 256, L[l].w + w_off0, L[l].ldw, 0, 256, acc, L[l].wpk, L[l].npk, r_off0);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int n = 16 * (c.wave * 2 + i) + 4 * c.fg;
                    const float4 b = *reinterpret_cast<const float4*>(L[l].b + b_off0 + n);
                    *reinterpret_cast<uint2*>(outb + c.fi * TK_AS + n * 2) =
                        make_uint2(pack_op16(fmaxf(acc[i][0][0] + b.x, 0.f), fmaxf(acc[i][0][1] + b.y, 0.f)), pack_op16(fmaxf(acc[i][0][2] + b.z, 0.f), fmaxf(acc[i][0][3] + b.w, 0.f)));
                }
                __syncthreads();
            }
            if (c.wave * 16 < n_out) {
                f32x4 acc[1][1];
                wgemm<1, 1>(c, c.H, 256, L[2].w + w_off2, L[2].ldw, 0, n_out, acc, L[2].wpk, L[2].npk, r_off2);
                if (c.fi < np) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int n = 16 * c.wave + 4 * c.fg + r;
                        if (n < n_out) {
                            float v = acc[0][0][r] + L[2].b[b_off2 + n];
                            if (sigmoid) v = 1.0f / (1.0f + __expf(-v));
                            out[(int64_t)(p0 + c.fi) * ldo + o_off + n] = v;
                        }
                    }
                }
            }
            __syncthreads();
        };
        mlp3(s.iou, 0, 0, 0, 0, 0, 0, 1, 4, 1, s.iou4, 4, 0);
        if (s.obj_out) mlp3(s.obj, 0, 0, 0, 0, 0, 0, 0, 1, 0, s.obj_out, 1, 0);
        for (int k = 0; k < 4; ++k)
            mlp3(s.hyper, (int64_t)k * 256 * s.hyper[0].ldw, (int64_t)k * 32 * s.hyper[2].ldw, 256 * k, 32 * k, 256 * k, 32 * k, 2 + k, 32, 0, s.hyper_out, 128, 32 * k);
    }
}

#define T16_TOK_LDS (TK_R * 256 * 4 + 3 * TK_R * TK_AS + 3 * TK_R * TK_FS * 4)
const char* launch_dec_tokens16(const TokSeg& s, int nvalid, hipStream_t st) {
    if (s.P <= 0) return nullptr;
    if (nvalid < 9 || nvalid > 16) return "dec_tokens16: 9..16 valid tokens per prompt";
    if (s.do_mlp && (!s.mlp1_pk || !s.mlp2_pk)) return "dec_tokens16: the MLP needs the K-step-packed copies of its two weights (launch_pack_w_kstep)";
    hipLaunchKernelGGL(dec_tokens16_kernel, dim3((s.P + T16_G - 1) / T16_G), dim3(TK_T), T16_TOK_LDS, st, s, nvalid);
    return nullptr;
}

// ------------------------------------------------------------------------------------------------ image -> tokens, 16 tokens per prompt
// X_out[p][n] = LN(x_n + softmax_heads((x_n + pe_n).Kt + cb).Vt + b_o) with 128 score columns c = 16 h + t: dec_i2t_kernel<1> (decoder_fused.hip)
// with wave qr owning the 32 columns of heads 2 qr and 2 qr + 1 (one 16-column tile per head: the softmax over a head's tokens stays inside
// the tile) and the 128 columns of P in GEMM2 (4 k-steps).  Same structure: 4 waves, 16-row tiles through a 4-stage LDS-DMA ring of X + PEQ,
// the folded operands in registers, one barrier per tile, normalisation of tile t after the barrier of tile t + 1.  The positional term
// k_h . PEQ_h is one MFMA per head with the operand [k_2qr | 0] or [0 | k_2qr+1] (k = 32 channels of the PEQ fragment).
#define T16_PEQ_ROWB 256                          // one PEQ row: 128 bf16
#define T16_NSTAGE 4
#define T16_ROWB 512                              // one X row: 256 bf16
#define T16_PSTRIDE 272                           // bytes per P row (128 bf16 + pad)
#define T16_STAGE (16 * T16_ROWB + 16 * T16_PEQ_ROWB)
#define T16_PBUF_B (16 * T16_PSTRIDE)
#define T16_STAT_B (16 * 4 * 2 * 4)
#define T16_CST_OFF (T16_NSTAGE * T16_STAGE + 2 * T16_PBUF_B + 2 * T16_STAT_B + 4 * 2048)
#define T16_LDS (T16_CST_OFF + 3 * 1024 + 512)     // + gamma | beta | b_o fp32 [256] each | score bias [128]: 69 KB, two workgroups per CU
#ifndef I2T16_X_AUX
#define I2T16_X_AUX 2                             // nontemporal read of a prompt's own X (its last use), as dec_i2t
#endif
typedef __attribute__((address_space(1))) const void* gptr16_d;
typedef __attribute__((address_space(3))) void* lptr16_d;
__device__ __forceinline__ void lds_write_b64_16(uint32_t addr, uint32_t lo, uint32_t hi) {
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ op16x8 pack8_t16(float a0, float a1, float a2, float a3, float b0, float b1, float b2, float b3) {
    const uint4 u = make_uint4(pack_op16(a0, a1), pack_op16(a2, a3), pack_op16(b0, b1), pack_op16(b2, b3));
    return __builtin_bit_cast(op16x8, u);
}
__device__ __forceinline__ int kswz16(int row, int chunk) { return row * T16_ROWB + ((chunk ^ (row & 15)) << 4); }

__global__ __launch_bounds__(256, 2) void dec_i2t16_kernel(const bf16_t* __restrict__ X, int64_t x_bs, int x_div, int x_off, const bf16_t* __restrict__ peq,
                                                           const bf16_t* __restrict__ Kt, const float* __restrict__ tk, float kscale, const float* __restrict__ cb,
                                                           const bf16_t* __restrict__ VtT, const float* __restrict__ bo,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           bf16_t* __restrict__ Xout, int nsplit, int nvalid) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* pbuf = smem + T16_NSTAGE * T16_STAGE;                         // [2][16 rows][272 B]
    float* stat = reinterpret_cast<float*>(pbuf + 2 * T16_PBUF_B);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qr = wave;
    const int fi = lane & 15, fg = lane >> 4;
    const int p = blockIdx.x / nsplit;
    const int NT = (4096 / 16) / nsplit;
    const int64_t row0 = (int64_t)(blockIdx.x % nsplit) * NT * 16;
    const bf16_t* Xp = X + (int64_t)((p + x_off) / x_div) * x_bs + row0 * T16_C;
    const bf16_t* pep = peq + row0 * 128;
    bf16_t* Xo = Xout + ((int64_t)p * 4096 + row0) * T16_C;

    // folded operands of this prompt, straight into registers: kf[j] = Kt rows 32 qr + 16 j + fi (head 2 qr + j, token fi)
    op16x8 kf[2][8], vf[4][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            kf[j][ks] = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(Kt + ((int64_t)p * 128 + 32 * qr + 16 * j + fi) * T16_C + 32 * ks + 8 * fg));
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            vf[t][ks] = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(VtT + ((int64_t)p * 256 + 64 * qr + 16 * t + fi) * 128 + 32 * ks + 8 * fg));
    op16x8 kq[2];   // projected keys of head 2 qr + j: row fi = token fi; k = 8 fg .. + 7 of [head 2 qr 16 | head 2 qr + 1 16], the other head zero
    {
        const int hsel = fg >> 1;
        const float* kp = tk + ((int64_t)p * 16 + fi) * 128 + 16 * (2 * qr + hsel) + 8 * (fg & 1);
        const float4 a = *reinterpret_cast<const float4*>(kp), b = *reinterpret_cast<const float4*>(kp + 4);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float z = (j == hsel && fi < nvalid) ? kscale : 0.f;
            kq[j] = pack8_t16(a.x * z, a.y * z, a.z * z, a.w * z, b.x * z, b.y * z, b.z * z, b.w * z);
        }
    }
    bool live[4];     // score rows 4 fg + r of a head tile are token 4 fg + r: valid keys only
#pragma unroll
    for (int r = 0; r < 4; ++r) live[r] = 4 * fg + r < nvalid;
    // gamma, beta and b_o wait in LDS (in registers, as dec_i2t keeps them, the twice-as-large folded operands would leave no room for a
    // second workgroup per CU); visible with the barrier in front of the tile loop
    {
        float* cst = reinterpret_cast<float*>(smem + T16_CST_OFF);
        cst[tid] = gamma[tid]; cst[256 + tid] = beta[tid]; cst[512 + tid] = bo[tid];
        if (tid < 128) cst[768 + tid] = cb[(int64_t)p * 128 + tid];
    }
    // direct-to-LDS: per stage 8 X wave-instructions (1 KB = 2 rows each; wave w issues 2 w, 2 w + 1) and 4 PEQ ones (4 rows of 256 B,
    // 16-B chunks XOR-swizzled by row & 15; wave w issues piece w)
    int srow[2], schunk[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        srow[i] = 2 * (wave * 2 + i) + (lane >> 5);
        schunk[i] = (lane & 31) ^ (srow[i] & 15);
    }
    const int prow = 4 * wave + (lane >> 4), pchunk = (lane & 15) ^ (prow & 15);
    auto issue = [&](int t) {
        char* sx = smem + (t & (T16_NSTAGE - 1)) * T16_STAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t off = (int64_t)(t * 16 + srow[i]) * T16_C + schunk[i] * 8;
            if (x_div > 1) __builtin_amdgcn_global_load_lds((gptr16_d)(Xp + off), (lptr16_d)(sx + (wave * 2 + i) * 1024), 16, 0, 0);
            else __builtin_amdgcn_global_load_lds((gptr16_d)(Xp + off), (lptr16_d)(sx + (wave * 2 + i) * 1024), 16, 0, I2T16_X_AUX);
        }
        __builtin_amdgcn_global_load_lds((gptr16_d)(pep + (int64_t)(t * 16 + prow) * 128 + pchunk * 8), (lptr16_d)(sx + 16 * T16_ROWB + wave * 1024), 16, 0, 0);
    };
    const int poff = fi * T16_PEQ_ROWB + (((4 * qr + fg) ^ fi) << 4);   // B fragment of the PEQ tile: row fi, columns 32 qr + 8 fg ..
    // B fragment of row fi, k-step ks in the swizzled tile: kswz16(fi, 4 ks + fg) = xo[ks & 3] + 256 (ks >> 2) (four registers, not eight)
    int xo[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) xo[b] = kswz16(fi, 4 * b + fg);
    int roff[4];      // residual: x[m][64 qr + 16 t + 4 fg .. +3]
#pragma unroll
    for (int t = 0; t < 4; ++t) roff[t] = fi * T16_ROWB + (((8 * qr + 2 * t + (fg >> 1)) ^ fi) << 4) + (fg & 1) * 8;
    const uint32_t prow_a = (uint32_t)(uintptr_t)(lptr16_d)(pbuf + fi * T16_PSTRIDE);
    const uint32_t stat_a = (uint32_t)(uintptr_t)(lptr16_d)(stat + (fi * 4) * 2);
    const uint32_t smem_a = (uint32_t)(uintptr_t)(lptr16_d)smem;
    const uint32_t oscr_a = smem_a + T16_NSTAGE * T16_STAGE + 2 * T16_PBUF_B + 2 * T16_STAT_B + wave * 2048;
    const uint32_t cst_a = smem_a + T16_CST_OFF + (64 * qr + 4 * fg) * 4;
    const uint32_t cb_a = smem_a + T16_CST_OFF + 3 * 1024 + (32 * qr + 4 * fg) * 4;     // score bias of columns 32 qr + 16 j + 4 fg .. + 3 at + 64 j bytes      // channels 64 qr + 16 t + 4 fg .. + 3 at + 64 t bytes
    // the lane's 4 x 4 values of one of the three vectors (0 gamma, 1 beta, 2 b_o)
    auto read_cst = [&](int which, f32x4 (&v)[4]) {
        const uint32_t a = cst_a + which * 1024;
        asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:64\n\tds_read_b128 %2, %4 offset:128\n\tds_read_b128 %3, %4 offset:192\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(a) : "memory");
    };
    f32x2 y2[8];                      // y of the previous tile (bias + residual added), normalised one barrier later
    auto finish_tile = [&](int tp) {
        f32x4 a, b;
        asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)" : "=&v"(a), "=&v"(b) : "v"(stat_a + (tp & 1) * T16_STAT_B) : "memory");
        const float tot = (a.x + a.z) + (b.x + b.z), tsq = (a.y + a.w) + (b.y + b.w);
        const float mean = tot * (1.0f / T16_C);
        const float rstd = __builtin_amdgcn_rsqf(fmaxf(tsq * (1.0f / T16_C) - mean * mean, 0.f) + eps);
        const f32x2 mean2 = (f32x2){mean, mean}, rstd2 = (f32x2){rstd, rstd};
        const uint32_t tb = oscr_a + fi * 128 + (fg & 1) * 8;
        f32x4 g4[4], be4[4];
        read_cst(0, g4); read_cst(1, be4);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const f32x2 v0 = ((y2[2 * tt] - mean2) * rstd2) * (f32x2){g4[tt][0], g4[tt][1]} + (f32x2){be4[tt][0], be4[tt][1]};
            const f32x2 v1 = ((y2[2 * tt + 1] - mean2) * rstd2) * (f32x2){g4[tt][2], g4[tt][3]} + (f32x2){be4[tt][2], be4[tt][3]};
            lds_write_b64_16(tb + (((2 * tt + (fg >> 1)) ^ (fi & 7)) << 4), pack_op16(v0.x, v0.y), pack_op16(v1.x, v1.y));
        }
        u32x4 o0, o1;
        asm volatile("s_waitcnt lgkmcnt(0)\n\tds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(o0), "=&v"(o1) : "v"(oscr_a + (lane >> 3) * 128 + (((lane & 7) ^ ((lane >> 3) & 7)) << 4)) : "memory");
        bf16_t* orow = Xo + (int64_t)(tp * 16 + (lane >> 3)) * T16_C + 64 * qr + 8 * (lane & 7);
        __builtin_nontemporal_store(o0, reinterpret_cast<u32x4*>(orow));
        __builtin_nontemporal_store(o1, reinterpret_cast<u32x4*>(orow + 8 * T16_C));
    };
    issue(0); issue(1); issue(2);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int t = 0; t < NT; ++t) {
        const char* xs = smem + (t & (T16_NSTAGE - 1)) * T16_STAGE;
        const char* ps = xs + 16 * T16_ROWB;
        // GEMM1 (swapped): S^T[c][m] = Kt[c].x[m] + Kt[c].pe[m] + cb[c] for this wave's 2 x 16 columns c
        f32x4 s[2], s1[2];
        {
            const op16x8 pf = *reinterpret_cast<const op16x8*>(ps + poff);
            asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:64\n\ts_waitcnt lgkmcnt(0)" : "=&v"(s[0]), "=&v"(s[1]) : "v"(cb_a) : "memory");
#pragma unroll
            for (int j = 0; j < 2; ++j) s1[j] = MFMA_16x16x32(kq[j], pf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 8; ks += 2) {
            const op16x8 xf0 = *reinterpret_cast<const op16x8*>(xs + xo[ks & 3] + 256 * (ks >> 2));
            const op16x8 xf1 = *reinterpret_cast<const op16x8*>(xs + xo[(ks + 1) & 3] + 256 * (ks >> 2));
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                s[j] = MFMA_16x16x32(kf[j][ks], xf0, s[j], 0, 0, 0);
                s1[j] = MFMA_16x16x32(kf[j][ks + 1], xf1, s1[j], 0, 0, 0);
            }
        }
        // softmax over the 16 tokens of a head: this lane's 4 values + lanes ^ 16, ^ 32; padding tokens take no part
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x4 v = s[j] + s1[j];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = live[r] ? v[r] : -INFINITY;
            float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
            mx = xor16_max(mx);
            mx = xor32_max(mx);
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = live[r] ? __builtin_amdgcn_exp2f(v[r] - mx) : 0.f; sum += v[r]; }
            sum = xor16_sum(sum);
            sum = xor32_sum(sum);
            const float inv = __builtin_amdgcn_rcpf(sum);
            lds_write_b64_16(prow_a + (t & 1) * T16_PBUF_B + (32 * qr + 16 * j + 4 * fg) * 2, pack_op16(v[0] * inv, v[1] * inv), pack_op16(v[2] * inv, v[3] * inv));
        }
        // tile t + 1 must have landed before the barrier (dec_i2t_kernel's count: behind L(t+1) stay [S(t-3)] L(t+2) [S(t-2)])
        if (t + 3 >= NT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (t < 2) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else if (t == 2) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();      // P(t) and stat(t-1) complete, tile t+1 visible, slot of tile t-1 free
        if (t + 3 < NT) issue(t + 3);
        if (t > 0) finish_tile(t - 1);
        // GEMM2: Y^T[d][m] for this wave's 64 channels over the 128 columns of P
        f32x4 y[4];
        {
            op16x8 pk[4];
            asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:64\n\tds_read_b128 %2, %4 offset:128\n\tds_read_b128 %3, %4 offset:192\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(pk[0]), "=&v"(pk[1]), "=&v"(pk[2]), "=&v"(pk[3]) : "v"(prow_a + (t & 1) * T16_PBUF_B + 16 * fg) : "memory");
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                y[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) y[tt] = MFMA_16x16x32(vf[tt][ks], pk[ks], y[tt], 0, 0, 0);
            }
        }
        uint64_t xr0, xr1, xr2, xr3;
        {
            const uint32_t xa = smem_a + (t & (T16_NSTAGE - 1)) * T16_STAGE;
            asm volatile("ds_read_b64 %0, %4\n\tds_read_b64 %1, %5\n\tds_read_b64 %2, %6\n\tds_read_b64 %3, %7\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(xr0), "=&v"(xr1), "=&v"(xr2), "=&v"(xr3)
                         : "v"(xa + roff[0]), "v"(xa + roff[1]), "v"(xa + roff[2]), "v"(xa + roff[3])
                         : "memory");
        }
        const uint64_t xrs[4] = {xr0, xr1, xr2, xr3};
        f32x4 bo4[4];
        read_cst(2, bo4);
        f32x2 sum2 = (f32x2){0.f, 0.f}, sq2 = (f32x2){0.f, 0.f};
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const uint32_t xlo = (uint32_t)xrs[tt], xhi = (uint32_t)(xrs[tt] >> 32);
            const f32x2 r0 = (f32x2){op16_lo(xlo), op16_hi(xlo)};
            const f32x2 r1 = (f32x2){op16_lo(xhi), op16_hi(xhi)};
            y2[2 * tt] = ((f32x2){y[tt][0], y[tt][1]} + (f32x2){bo4[tt][0], bo4[tt][1]}) + r0;
            y2[2 * tt + 1] = ((f32x2){y[tt][2], y[tt][3]} + (f32x2){bo4[tt][2], bo4[tt][3]}) + r1;
            sum2 += y2[2 * tt]; sum2 += y2[2 * tt + 1];
            sq2 = __builtin_elementwise_fma(y2[2 * tt], y2[2 * tt], sq2);
            sq2 = __builtin_elementwise_fma(y2[2 * tt + 1], y2[2 * tt + 1], sq2);
        }
        float sum = sum2.x + sum2.y, sq = sq2.x + sq2.y;
        sum = xor16_sum(sum); sq = xor16_sum(sq);
        sum = xor32_sum(sum); sq = xor32_sum(sq);
        if (fg == 0) lds_write_b64_16(stat_a + (t & 1) * T16_STAT_B + qr * 8, __float_as_uint(sum), __float_as_uint(sq));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    finish_tile(NT - 1);
}

const char* launch_dec_i2t16(const bf16_t* X, XMap xm, const bf16_t* peq, const bf16_t* Kt, const float* tk, float kscale, const float* cb, const bf16_t* VtT,
                             const float* bo, const float* gamma, const float* beta, float eps, bf16_t* Xout, int P, int nvalid, hipStream_t s) {
    if (P <= 0) return nullptr;
    if (xm.div <= 0) return "dec_i2t16: XMap.div must be positive";
    if (nvalid < 1 || nvalid > 16) return "dec_i2t16: 1..16 valid tokens per prompt";
    int nsplit = 1;
    while (P * nsplit < 512 && nsplit < 8) nsplit *= 2;   // small batches: split a prompt's tiles over several blocks
    hipLaunchKernelGGL(dec_i2t16_kernel, dim3(P * nsplit), dim3(256), T16_LDS, s, X, xm.stride, xm.div, xm.off, peq, Kt, tk, kscale, cb, VtT, bo, gamma, beta, eps,
                       Xout, nsplit, nvalid);
    return nullptr;
}

const char* decoder_t16_init_device() {
    hipError_t st = hipFuncSetAttribute(reinterpret_cast<const void*>(dec_tokens16_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, T16_TOK_LDS);
    if (st == hipSuccess) st = hipFuncSetAttribute(reinterpret_cast<const void*>(dec_i2t16_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, T16_LDS);
    return st == hipSuccess ? nullptr : hipGetErrorString(st);
}
