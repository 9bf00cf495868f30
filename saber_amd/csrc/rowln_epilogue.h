// Epilogue shared by the row-owner kernels (gemm_rowln.hip, gemm_mlp_rowln.hip): a workgroup of 8 waves holds whole rows of
//     acc = A . W^T                                 (fp32 accumulators, 16x16 MFMA tiles: NI row tiles x 9 column tiles per wave)
// and finishes the Hiera residual step and the LayerNorm that follows it:
//     y  = acc + bias + res                         (fp32 -> Cf)
//     [Cb = rnd16(y)]
//     ln_out = rnd16(LayerNorm(y) * gamma + beta)
// Included inside the operand-type namespace of its includer (op_wrap.hip); no include guard beyond #pragma once: one includer per object.
#pragma once
#include "common.h"
#include "kernels.h"

typedef __attribute__((address_space(1))) const void* gptr_r;
typedef __attribute__((address_space(3))) void* lptr_r;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

#define RL_PITCH 304                 // bytes per row of the bf16 transposition scratch (288 + 16)
#define RL_SCR (16 * RL_PITCH)       // per wave
// The timing-only switches of tools/rowln_bench.py (DBG=1024|2048|4096|8192|32768, the late-start sweep) exist in development builds only
// (make EXTRA=-DRL_DEV=1 BUILD=build_dev LIB=...): as run-time tests inside the K loop they cost a live register and a branch around every
// MFMA group, which pushed the fp16 build of the <2,4> configuration into spilling inside the loop.
#ifndef RL_DEV
#define RL_DEV 0
#endif
#define RL_DBG(bit) (RL_DEV && (p.dbg & (bit)))

// Lane owns rows m0 + wm * 16 NI + i * 16 + fi, columns wn * 144 + j * 16 + fg * 4 .. + 3 (fi = lane & 15, fg = lane >> 4) of a tile of R rows x
// 144 WN columns.  stat0: two buffers of R x WN floats in LDS (the partial row sums of the WN waves of a row; unused with WN = 1); scr: 8 x RL_SCR
// bytes of LDS, wave-private.  mid() runs once every wave is done with the accumulators' fp32 form, ahead of the statistics and the 16-bit stores:
// the place to put the next tile's first loads in flight.  All LDS traffic and barriers in here are inline asm / raw, so that loads the caller
// has in flight (direct-to-LDS or not) are never drained by a compiler-inserted vmcnt(0).
template <int NI, int WN, int R, class Mid>
__device__ __forceinline__ void rowln_epilogue(const GemmParams& p, f32x4 (&acc)[NI][9], int m0, int wm, int wn, int wave, int lane, float* stat0, char* scr_base, Mid&& mid) {
    constexpr int N = 144 * WN;
    // (opaque lane copy: keeps the epilogue's address arithmetic from being hoisted above the main loop, where every live register
    // costs a spill).  Residual, fp32 rows and bf16 rows go through buffer descriptors over this tile's rows: one 32-bit offset per
    // lane and tensor, the row group in the scalar offset, the column group in the immediate; rows beyond M are dropped by the range check.
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    const int efi = lane_e & 15, efg = lane_e >> 4;
    const int ncol = wn * 144 + efg * 4;
    const int trow = wm * (16 * NI) + efi;                // row within the tile (+ 16 i)
    const int rows = min(R, p.M - m0);
    const float* rbase = p.res ? p.res : p.Cf;            // no residual: any readable fp32 (discarded)
    const int64_t ldr = p.res ? p.ldres : p.ldcf;
    const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(rbase + (int64_t)m0 * ldr), 0, (int)((uint32_t)rows * (uint32_t)ldr * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t crsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.Cf + (int64_t)m0 * p.ldcf), 0, (int)((uint32_t)rows * (uint32_t)p.ldcf * 4u), 0x00020000);
    const uint32_t roff = (uint32_t)((trow * (int)ldr + ncol) * 4), coff = (uint32_t)((trow * (int)p.ldcf + ncol) * 4);
    const uint32_t rstep = (uint32_t)(16 * (int)ldr * 4), cstep = (uint32_t)(16 * (int)p.ldcf * 4);
    const bool has_res = p.res != nullptr;
    const bool dbg_nores = RL_DBG(1024), dbg_nof32 = RL_DBG(2048), dbg_nobf = RL_DBG(4096);   // development: timing-only switches (tools/rowln_bench.py)
    // No direct-to-LDS load is in flight here (the callers' main loops end with everything landed), so hipcc counts these loads instead of
    // draining the queue at every use; the residual rows of group i + 1 are requested before group i is added and stored.
    u32x4 ra[9], rb[9];
    auto load_group = [&](const __amdgpu_buffer_rsrc_t& rsr, int i, u32x4 (&rr)[9]) {
#pragma unroll
        for (int j = 0; j < 9; ++j) rr[j] = dbg_nores ? (u32x4){0u, 0u, 0u, 0u} : __builtin_amdgcn_raw_buffer_load_b128(rsr, roff + j * 64, i * rstep, 0);
    };
    float rs[NI];
    auto finish_group = [&](const __amdgpu_buffer_rsrc_t& csr, int i, const u32x4 (&rr)[9]) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            if (has_res) {
                acc[i][j][0] += __uint_as_float(rr[j][0]); acc[i][j][1] += __uint_as_float(rr[j][1]);
                acc[i][j][2] += __uint_as_float(rr[j][2]); acc[i][j][3] += __uint_as_float(rr[j][3]);
            }
            s += (acc[i][j][0] + acc[i][j][1]) + (acc[i][j][2] + acc[i][j][3]);
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            u32x4 v;
            v[0] = __float_as_uint(acc[i][j][0]); v[1] = __float_as_uint(acc[i][j][1]); v[2] = __float_as_uint(acc[i][j][2]); v[3] = __float_as_uint(acc[i][j][3]);
            if (!dbg_nof32) __builtin_amdgcn_raw_buffer_store_b128(v, csr, coff + j * 64, i * cstep, 0);
        }
        rs[i] = xor32_sum(xor16_sum(s));
    };
    load_group(rrsrc, 0, ra);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const float4 b4 = p.bias ? *reinterpret_cast<const float4*>(p.bias + ncol + j * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < NI; ++i) { acc[i][j][0] += b4.x; acc[i][j][1] += b4.y; acc[i][j][2] += b4.z; acc[i][j][3] += b4.w; }
    }
    __builtin_amdgcn_sched_barrier(0);
    // group i + 1 is requested (into the buffer group i - 1 has left) before group i is added and stored
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if (i + 1 < NI) {
            if (i & 1) load_group(rrsrc, i + 1, ra); else load_group(rrsrc, i + 1, rb);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (i & 1) finish_group(crsrc, i, rb); else finish_group(crsrc, i, ra);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (p.Cb) {
        const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.Cb + (int64_t)m0 * p.ldcb), 0, (int)((uint32_t)rows * (uint32_t)p.ldcb * 2u), 0x00020000);
        const uint32_t boff = (uint32_t)((trow * (int)p.ldcb + ncol) * 2), bstep = (uint32_t)(16 * (int)p.ldcb * 2);
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                u32x2 v;
                v[0] = pack_op16(acc[i][j][0], acc[i][j][1]); v[1] = pack_op16(acc[i][j][2], acc[i][j][3]);
                __builtin_amdgcn_raw_buffer_store_b64(v, brsrc, boff + j * 32, i * bstep, 0);
            }
    }
    mid();
    // mean / variance over the N columns of each row: the partial sums of the WN waves of a row meet in LDS.  LDS traffic and the
    // barrier are inline asm / raw: a visible ds access or __syncthreads() would drain the direct-to-LDS loads and all stores (vmcnt(0)).
    float mean[NI], rstd[NI];
    const uint32_t st_w = (uint32_t)(uintptr_t)(lptr_r)stat0 + (uint32_t)((trow * WN + wn) * 4);   // this wave's slot of row trow (+ 16 i rows)
    const uint32_t st_r = (uint32_t)(uintptr_t)(lptr_r)stat0 + (uint32_t)(trow * WN * 4);
    auto exchange = [&](int buf, float (&v)[NI]) {        // v[i] <- sum over the WN waves of the row
        if (WN == 1) return;
        const uint32_t bo = (uint32_t)(buf * R * WN * 4);
        if (efg == 0) {
#pragma unroll
            for (int i = 0; i < NI; ++i) asm volatile("ds_write_b32 %0, %1" ::"v"(st_w + bo + i * 16 * WN * 4), "v"(v[i]) : "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (WN == 4) {
                f32x4 q4;
                asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(q4) : "v"(st_r + bo + i * 16 * WN * 4) : "memory");
                v[i] = (q4[0] + q4[1]) + (q4[2] + q4[3]);
            } else {
                f32x2 q2;
                asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(q2) : "v"(st_r + bo + i * 16 * WN * 4) : "memory");
                v[i] = q2[0] + q2[1];
            }
        }
    };
    exchange(0, rs);
#pragma unroll
    for (int i = 0; i < NI; ++i) mean[i] = rs[i] * (1.0f / N);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { acc[i][j][r] -= mean[i]; q = fmaf(acc[i][j][r], acc[i][j][r], q); }
        rs[i] = xor32_sum(xor16_sum(q));
    }
    exchange(1, rs);
#pragma unroll
    for (int i = 0; i < NI; ++i) rstd[i] = __builtin_amdgcn_rsqf(rs[i] * (1.0f / N) + p.ln_eps);
    const __amdgpu_buffer_rsrc_t lrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ln_out + (int64_t)m0 * p.ldln), 0, (int)((uint32_t)rows * (uint32_t)p.ldln * 2u), 0x00020000);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const float4 g4 = *reinterpret_cast<const float4*>(p.ln_gamma + ncol + j * 16);
        const float4 be4 = *reinterpret_cast<const float4*>(p.ln_beta + ncol + j * 16);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            acc[i][j][0] = fmaf(acc[i][j][0] * rstd[i], g4.x, be4.x); acc[i][j][1] = fmaf(acc[i][j][1] * rstd[i], g4.y, be4.y);
            acc[i][j][2] = fmaf(acc[i][j][2] * rstd[i], g4.z, be4.z); acc[i][j][3] = fmaf(acc[i][j][3] * rstd[i], g4.w, be4.w);
        }
    }
    // bf16 rows leave through LDS: in the accumulator layout a store instruction covers 16 rows x 32 B (the same bytes cost twice
    // what the fp32 rows cost: tools/rowln_bench.py, DBG=4096 against DBG=2048); transposed, a lane stores 16 B of a 288-B row
    // segment, 3 rows per instruction.  The scratch is wave-private (16 rows x 304 B: the pitch spreads the 16 rows of a
    // ds_write_b64 over the banks).
    const uint32_t scr = (uint32_t)(uintptr_t)(lptr_r)scr_base + (uint32_t)(wave * RL_SCR);
    const uint32_t scr_w = scr + (uint32_t)(efi * RL_PITCH + efg * 8);
    const int lrow = lane_e / 18, lch = lane_e - 18 * lrow;                  // lanes 0..53: 3 rows x 18 chunks of 16 B
    const uint32_t scr_r = scr + (uint32_t)(lrow * RL_PITCH + lch * 16);
    const uint32_t loff = (uint32_t)(((wm * (16 * NI) + lrow) * (int)p.ldln + wn * 144) * 2 + lch * 16);
    const uint32_t lrowb = (uint32_t)((int)p.ldln * 2);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const uint64_t pk = ((uint64_t)pack_op16(acc[i][j][2], acc[i][j][3]) << 32) | pack_op16(acc[i][j][0], acc[i][j][1]);
            asm volatile("ds_write_b64 %0, %1" ::"v"(scr_w + j * 32), "v"(pk) : "memory");
        }
        u32x4 val[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) asm volatile("ds_read_b128 %0, %1" : "=v"(val[r]) : "v"(scr_r + r * 3 * RL_PITCH) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(val[0]), "+v"(val[1]), "+v"(val[2]), "+v"(val[3]), "+v"(val[4]), "+v"(val[5]));
        if (!dbg_nobf && lane_e < 54) {
#pragma unroll
            for (int r = 0; r < 5; ++r) __builtin_amdgcn_raw_buffer_store_b128(val[r], lrsrc, loff, (i * 16 + r * 3) * lrowb, 0);
            if (lane_e < 18) __builtin_amdgcn_raw_buffer_store_b128(val[5], lrsrc, loff, (i * 16 + 15) * lrowb, 0);
        }
    }
}
